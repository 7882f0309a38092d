"""Test helper: numpy reference of lbbnn_gate_structure / evaluate.structure_posterior, written straight from the semantics in
include/lbbnn.h.  ``structure_ref`` takes the gate arrays themselves; ``gate_uniforms`` / ``gates_ref`` build them on the CPU from
tests/philox_ref.py (the kernels' Philox keying and counters, the ((bits >> 8) + 0.5) 2^-24 map).  Not part of the product."""
import numpy as np

import philox_ref as pr

STREAM_GATE = 8          # LBBNN_STREAM_GATE


def gate_uniforms(seed, offset, layer_id, rows, cols):
    """(rows, cols) fp32: element (o, i) = word i % 4 of Philox counter (o, i // 4) of stream STREAM_GATE * 64 + layer_id at
    state {seed, offset}, as ((bits >> 8) + 0.5) 2^-24 (exact in fp32)."""
    g = (cols + 3) // 4
    o = np.arange(rows, dtype=np.uint64)[:, None] * np.ones((1, g), dtype=np.uint64)
    cg = np.ones((rows, 1), dtype=np.uint64) * np.arange(g, dtype=np.uint64)[None, :]
    k0, k1 = pr.key_of(seed, offset)
    stream = np.full(o.shape, STREAM_GATE * 64 + layer_id, np.uint64)
    words = pr.philox4x32_10(o & np.uint64(pr.MASK), o >> np.uint64(32), cg, stream, k0, k1)
    bits = np.stack(words, axis=-1).reshape(rows, 4 * g)[:, :cols]
    return (((bits >> np.uint64(8)).astype(np.float64) + 0.5) * 2.0 ** -24).astype(np.float32)


def gates_ref(alphas, layer_ids, seed, offset, samples):
    """Per layer the (samples, O, I) bool gates u < alpha; sample s draws at offset + s.  ``alphas``: (O, I) arrays (fp32 for
    the device's own comparison, fp64 for an independent one).  Also returns per layer the (samples, O, I) |u - alpha|."""
    gates, dist = [], []
    for al, lid in zip(alphas, layer_ids):
        O, I = al.shape
        u = np.stack([gate_uniforms(seed, offset + s, lid, O, I) for s in range(samples)])
        gates.append(u.astype(al.dtype) < al[None])
        dist.append(np.abs(u.astype(np.float64) - al[None].astype(np.float64)))
    return gates, dist


def structure_ref(gates):
    """``gates``: per layer a (S, O, I) (or (O, I)) bool array, first layer first.  Returns a dict: kept (S, n), need (per
    boundary (S, width) bool), needed (S, n + 1), active_kept (S, n), feature_count (I0,), unit_count (per hidden boundary)."""
    gates = [np.asarray(g, dtype=bool) for g in gates]
    gates = [g[None] if g.ndim == 2 else g for g in gates]
    n, S = len(gates), gates[0].shape[0]
    kept = np.zeros((S, n), np.int64)
    active = np.zeros((S, n), np.int64)
    need = [None] * (n + 1)
    need[n] = np.ones((S, gates[-1].shape[1]), bool)
    for l in range(n - 1, -1, -1):
        g = gates[l]
        assert g.shape[1] == need[l + 1].shape[1], "layer %d: rows do not match the boundary above" % l
        live = g & need[l + 1][:, :, None]                   # the kept weights of needed rows
        need[l] = live.any(axis=1)
        kept[:, l] = g.sum(axis=(1, 2))
        active[:, l] = live.sum(axis=(1, 2))
    needed = np.stack([nd.sum(axis=1) for nd in need], axis=1).astype(np.int64)
    return {"kept": kept, "need": need, "needed": needed, "active_kept": active,
            "feature_count": need[0].sum(axis=0).astype(np.int64),
            "unit_count": [need[b].sum(axis=0).astype(np.int64) for b in range(1, n)]}
