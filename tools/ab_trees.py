"""What the byte-comparison tools share (eval_totals_ab.py, train_loss_ab.py): run a tool's worker once per tree, collect the
dumps, compare them key by key.

A tool is a script with ``--worker TREE --dump FILE``: the worker puts TREE first on the import path, runs its cases on the
device and pickles ``{"<case>[ #<n>]/<array>": bytes}`` into FILE.  ``child_dumps`` starts it for a built checkout of the
parent commit and for this tree, each in a fresh child process under its own time limit, and stops at the first child that
fails; the calling process never touches the device.  ``report`` prints and writes ``identical`` or the first key that differs,
per case, and returns the exit status."""
import os
import pickle
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child_dumps(tool, parent, timeout, extra=(), env=None):
    """{"parent": dump, "this tree": dump} of ``tool`` (its ``__file__``); ``extra``: further arguments of the workers,
    ``env``: variables set for them."""
    stem = os.path.splitext(os.path.basename(tool))[0]
    dumps = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, tree in (("parent", os.path.abspath(parent)), ("this tree", HERE)):
            path = os.path.join(tmp, name.replace(" ", "_") + ".pkl")
            child_env = {k: v for k, v in os.environ.items() if k != "LBBNN_LIB_PATH"}      # each tree loads its own library
            child_env.update(env or {})
            rc = subprocess.run(["timeout", "-k", "10", str(timeout), sys.executable, os.path.abspath(tool),
                                 "--worker", tree, "--dump", path, *extra], env=child_env, cwd=tree).returncode
            if rc != 0 or not os.path.exists(path):
                sys.exit("%s: the child of %s (%s) ended with status %d; stopped" % (stem, name, tree, rc))
            with open(path, "rb") as fh:
                dumps[name] = pickle.load(fh)
    return dumps


def report(tool, dumps, parent, out):
    """Compare the two dumps case by case (a case: the key up to its "/", without a " #<n>" suffix); print the lines, write
    them to ``out``; 0 when every case is identical, else 1."""
    a, b = dumps["parent"], dumps["this tree"]
    lines = []
    say = lambda s: (lines.append(s), print(s, flush=True))
    cases = {}
    for k in list(a) + [k for k in b if k not in a]:
        cases.setdefault(k.split("/")[0].rsplit(" #", 1)[0], []).append(k)
    bad = 0
    say("tools/%s: %d cases, %d dumped arrays (%d bytes); parent %s" % (os.path.basename(tool), len(cases), len(a),
                                                                       sum(map(len, a.values())), parent))
    for case, keys in cases.items():
        diff = next((k for k in keys if a.get(k) != b.get(k)), None)
        bad += diff is not None
        say("%-78s %s" % (case, "identical" if diff is None else "DIFFERENT at %s" % diff))
    say("every case identical" if not bad else "%d case(s) DIFFERENT" % bad)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return 1 if bad else 0
