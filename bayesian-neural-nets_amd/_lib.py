"""ctypes binding of the C ABI in include/lbbnn.h.

There is deliberately NO fallback: if ``csrc/liblbbnn_hip.so`` is missing, or a tensor is not on
a HIP device, the call raises.  (The CPU oracle under ``oracle/`` is test infrastructure and is
never imported from here.)
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# LBBNN_LIB_PATH: developer hook for the ablation builds of tools/lab (must exist; still no fallback)
LIB_PATH = os.environ.get("LBBNN_LIB_PATH") or os.path.join(_HERE, "csrc", "liblbbnn_hip.so")

c_p = ctypes.c_void_p
c_i = ctypes.c_int
c_u32 = ctypes.c_uint32
c_i64 = ctypes.c_int64
c_u64 = ctypes.c_uint64


class Priors(ctypes.Structure):
    """lbbnn_priors_t (include/lbbnn.h)."""
    _fields_ = [("mu_prior", ctypes.c_float), ("sigma_prior", ctypes.c_float),
                ("alpha_prior", ctypes.c_float), ("bias_mu_prior", ctypes.c_float),
                ("bias_sigma_prior", ctypes.c_float)]

    def __init__(self, mu_prior=0.0, sigma_prior=1.0, alpha_prior=0.05, bias_mu_prior=0.0,
                 bias_sigma_prior=1.0):
        super().__init__(mu_prior, sigma_prior, alpha_prior, bias_mu_prior, bias_sigma_prior)


MAX_FLOW_T = 16
MAX_LAYERS = 4            # LBBNN_MAX_LAYERS: layers per batched launch
MAX_DEPTH = 16            # LBBNN_MAX_DEPTH: layers per network (Philox stream ids are kind * 64 + layer id)


def layer_groups(n: int):
    """[(first layer, count)] of the ceil(n / MAX_LAYERS) groups of consecutive layers in which a network of n layers issues
    its batched C calls (every struct array of such a call holds MAX_LAYERS entries)."""
    return [(k, min(MAX_LAYERS, n - k)) for k in range(0, n, MAX_LAYERS)]


def group_slice(arr, first: int, count: int):
    """Entries first .. first + count - 1 of a ctypes struct array as an array of their own over the SAME memory (the view
    keeps ``arr`` alive): what a group's call is given."""
    if first == 0 and count == len(arr):
        return arr
    return (arr._type_ * count).from_buffer(arr, first * ctypes.sizeof(arr._type_))


class PlanarFlow(ctypes.Structure):
    """lbbnn_planar_flow_t"""
    _fields_ = [("u", c_p * MAX_FLOW_T), ("w", c_p * MAX_FLOW_T), ("b", c_p * MAX_FLOW_T), ("T", c_i)]


class LayerDesc(ctypes.Structure):
    """lbbnn_layer_desc_t (field order must match include/lbbnn.h)"""
    _fields_ = [("weight_mu", c_p), ("weight_rho", c_p), ("lambdal", c_p), ("bias_mu", c_p), ("bias_rho", c_p),
                ("q0_mean", c_p), ("q0_log_var", c_p), ("r0_c", c_p), ("r0_b1", c_p), ("r0_b2", c_p),
                ("z_flow", PlanarFlow), ("r_flow", PlanarFlow), ("priors", Priors),
                ("O", c_i), ("I", c_i), ("layer_id", c_u32), ("stochastic", c_i), ("want_kl", c_i), ("split", c_i),
                ("eps_z", c_p), ("eps_z2", c_p), ("eps_act", c_p),
                ("z_fwd", c_p), ("z_kl", c_p), ("scal", c_p), ("e_w", c_p), ("var_w", c_p),
                ("kl_rows", c_p), ("act_mu", c_p), ("act_var", c_p), ("bias_var", c_p), ("kl_layer", c_p),
                ("flows_done", c_i), ("e_scale", c_p), ("v_scale", c_p)]


class GemmDesc(ctypes.Structure):
    """lbbnn_gemm_desc_t"""
    _fields_ = [("x", c_p), ("ldx", c_i), ("e_w", c_p), ("var_w", c_p), ("ld", c_i),
                ("mean_scale", c_p), ("wvar_scale", c_p), ("bias_mean", c_p), ("bias_var", c_p), ("var_scale", c_p),
                ("eps", c_p), ("rng", c_p), ("rng_stream", c_u32), ("row_offset", c_i64),
                ("out", c_p), ("ldo", c_i), ("out_planes", c_p), ("ldp", c_i), ("std_out", c_p),
                ("B", c_i), ("I", c_i), ("O", c_i), ("flags", c_i),
                ("layers", ctypes.POINTER(LayerDesc)), ("n_layers", c_i), ("fin_rng", c_p), ("kl_total", c_p),
                ("rng_live", c_p), ("advance", c_u64),
                ("head_e", c_p), ("head_v", c_p), ("head_ld", c_i), ("head_classes", c_i),
                ("head_bias_mean", c_p), ("head_bias_var", c_p), ("head_eps", c_p), ("head_rng_stream", c_u32),
                ("head_out", c_p), ("head_ldo", c_i), ("head_slab", c_p), ("head_flags", c_i)]


class GemmPlan(ctypes.Structure):
    """lbbnn_gemm_plan_t"""
    _fields_ = [("family", c_i), ("large_tile", c_i), ("xvec", c_i), ("mean_only", c_i), ("products", c_i), ("half", c_i),
                ("fan", c_i), ("kernel_id", c_i)]


GEMM_FAMILIES = {-1: "none", 0: "skinny", 1: "staged", 2: "dma", 3: "split"}      # LBBNN_GEMM_*


class DenseTransform(ctypes.Structure):
    """lbbnn_dense_transform_t"""
    _fields_ = [("kind", c_i), ("hidden", c_i), ("w_in", c_p), ("b_in", c_p),
                ("w_mid", c_p * 3), ("b_mid", c_p * 3), ("w_a", c_p), ("b_a", c_p), ("w_b", c_p), ("b_b", c_p),
                ("mask_fwd", c_p), ("mask_kl", c_p)]


class GateArgs(ctypes.Structure):
    """lbbnn_gate_args_t"""
    _fields_ = [(n, c_p) for n in ("mu", "rho", "gamma_alpha", "cgamma", "eps_w", "alpha_attr",
                                   "bias_mu", "bias_rho", "eps_b", "bias_a", "bias_b", "tau_b",
                                   "weight_a", "weight_b", "tau_w", "pa", "pb",
                                   "w_out", "bias_out", "rows", "log_prior", "log_q")] + \
               [(n, c_i) for n in ("O", "I", "ld", "mode", "exact", "want_lp", "flags")] + [("layer_id", c_u32)]


class ReduceJob(ctypes.Structure):
    """lbbnn_reduce_job_t (include/lbbnn.h)."""
    _fields_ = [("work", c_p), ("out", c_p * 3), ("block_stride", ctypes.c_int64), ("q_stride", ctypes.c_int64),
                ("nblk", c_i), ("ncols", c_i), ("nq", c_i)]


class AuxBwdArgs(ctypes.Structure):
    """lbbnn_aux_bwd_args_t (include/lbbnn.h)."""
    _fields_ = [(n, c_p) for n in ("act_mu", "act_var", "eps_act", "r0_b1", "r0_b2", "zb_last", "g_kl", "da_mu", "da_var", "aux",
                                   "rng")] + [("O", c_i), ("I", c_i), ("layer_id", ctypes.c_uint32)]


class WpbArgs(ctypes.Structure):
    """lbbnn_wpb_args_t"""
    _fields_ = [(n, c_p) for n in ("mu", "rho", "lambdal", "dWm", "dWv", "z_fwd", "z_kl", "r0_c",
                                   "da_mu", "da_var", "g_kl")] + [("priors", Priors)] + \
               [(n, c_p) for n in ("dmu", "drho", "dlambdal", "dz_fwd", "dz_kl", "dr0_c", "work")] + \
               [("O", c_i), ("I", c_i), ("nsplit", c_i), ("split_stride", c_i64)]


ADAM_MAX_TENSORS = 80


class AdamList(ctypes.Structure):
    """lbbnn_adam_list_t"""
    _fields_ = [("p", c_p * ADAM_MAX_TENSORS), ("g", c_p * ADAM_MAX_TENSORS), ("m", c_p * ADAM_MAX_TENSORS),
                ("v", c_p * ADAM_MAX_TENSORS), ("numel", c_i64 * ADAM_MAX_TENSORS), ("n", c_i)]


ADAM_GROUPS_MAX_TENSORS = 64
ADAM_CHUNK = 4096                      # LBBNN_ADAM_CHUNK: elements per workgroup of the list kernels = per partial of lbbnn_grad_sumsq
ADAM_F_DECOUPLED = 0x1
ADAM_F_INACTIVE = 0x2


class AdamHyper(ctypes.Structure):
    """lbbnn_adam_hyper_t: one row of the device table (6 x 4 bytes)"""
    _fields_ = [("lr", ctypes.c_float), ("beta1", ctypes.c_float), ("beta2", ctypes.c_float), ("eps", ctypes.c_float),
                ("weight_decay", ctypes.c_float), ("flags", c_u32)]


class AdamGroupList(ctypes.Structure):
    """lbbnn_adam_group_list_t"""
    _fields_ = [("p", c_p * ADAM_GROUPS_MAX_TENSORS), ("g", c_p * ADAM_GROUPS_MAX_TENSORS), ("m", c_p * ADAM_GROUPS_MAX_TENSORS),
                ("v", c_p * ADAM_GROUPS_MAX_TENSORS), ("mask", c_p * ADAM_GROUPS_MAX_TENSORS),
                ("numel", c_i64 * ADAM_GROUPS_MAX_TENSORS), ("group", c_i * ADAM_GROUPS_MAX_TENSORS), ("n", c_i)]


SGD_F_NESTEROV = 0x1
SGD_F_INACTIVE = 0x2


class SgdHyper(ctypes.Structure):
    """lbbnn_sgd_hyper_t: one row of the device table (5 x 4 bytes)"""
    _fields_ = [("lr", ctypes.c_float), ("momentum", ctypes.c_float), ("dampening", ctypes.c_float),
                ("weight_decay", ctypes.c_float), ("flags", c_u32)]


class StudyArgs(ctypes.Structure):
    """lbbnn_study_args_t"""
    _fields_ = [("params", c_p), ("exp_avg", c_p), ("exp_avg_sq", c_p), ("step", c_p), ("rng", c_p), ("skipped", c_p),
                ("x", c_p), ("x_rstride", c_i64), ("y", c_p), ("y_rstride", c_i64), ("priors", c_p), ("priors_rstride", c_i),
                ("hyper", c_p), ("lr", c_p), ("lr_rstride", c_i64), ("restarts", c_p), ("n_restarts", c_i), ("history", c_p),
                ("R", c_i), ("I", c_i), ("O", c_i), ("N", c_i), ("batch", c_i),
                ("epochs", c_i), ("first_epoch", c_i), ("n_epochs", c_i)]


class MnfStudyArgs(ctypes.Structure):
    """lbbnn_mnf_study_args_t: lbbnn_study_args_t's members, then the transform counts of the two flows"""
    _fields_ = list(StudyArgs._fields_) + [("Tz", c_i), ("Tr", c_i)]


STUDY_MAX_I, STUDY_MAX_O, STUDY_MAX_WEIGHTS, STUDY_MAX_BATCH, STUDY_HISTORY_COLS = 256, 16, 1024, 4096, 6     # LBBNN_STUDY_*
STUDY_MAX_TRANSFORMS = 4


class CopyList(ctypes.Structure):
    """lbbnn_copy_list_t"""
    _fields_ = [("dst", c_p * ADAM_MAX_TENSORS), ("src", c_p * ADAM_MAX_TENSORS), ("numel", c_i64 * ADAM_MAX_TENSORS), ("n", c_i)]


class DenseLayer(ctypes.Structure):
    """lbbnn_dense_layer_t"""
    _fields_ = [("q0_mean", c_p), ("q0_log_var", c_p), ("zt", ctypes.POINTER(DenseTransform)), ("rt", ctypes.POINTER(DenseTransform)),
                ("eps_fwd", c_p), ("eps_kl", c_p), ("z_fwd", c_p), ("z_kl", c_p), ("scal", c_p), ("work", c_p),
                ("Tz", c_i), ("Tr", c_i), ("I", c_i), ("want_kl", c_i), ("layer_id", c_u32), ("save", c_p), ("draw_masks", c_i)]


class DenseGrad(ctypes.Structure):
    """lbbnn_dense_grad_t"""
    _fields_ = [("w_in", c_p), ("b_in", c_p), ("w_mid", c_p * 3), ("b_mid", c_p * 3),
                ("w_a", c_p), ("b_a", c_p), ("w_b", c_p), ("b_b", c_p)]


MAX_DENSE_T = 8
MAX_HIDDEN = 128


class GateBwdArgs(ctypes.Structure):
    """lbbnn_gate_bwd_args_t"""
    _fields_ = [(n, c_p) for n in ("mu", "rho", "gamma_alpha", "cgamma", "eps_w", "bias_mu", "bias_rho", "eps_b", "bias_a",
                                   "bias_b", "tau_b", "weight_a", "weight_b", "tau_w", "pa", "pb", "dW", "g_sum", "g_lp", "g_lq",
                                   "d_mu", "d_rho", "d_cgamma", "d_alpha", "w_out", "d_bias_mu", "d_bias_rho", "d_bias_a",
                                   "d_bias_b", "d_tau_b", "d_scalars", "rows")] + \
               [("O", c_i), ("I", c_i), ("exact", c_i), ("layer_id", c_u32)]


class GateDrawArgs(ctypes.Structure):
    """lbbnn_gate_draw_args_t"""
    _fields_ = [("g", GateArgs), ("lambdal", c_p), ("gammas", c_p), ("alpha", c_p), ("tau_w", c_p), ("tau_b", c_p),
                ("temperature", ctypes.c_float)]


class GateBwdDrawArgs(ctypes.Structure):
    """lbbnn_gate_bwd_draw_args_t"""
    _fields_ = [("g", GateBwdArgs), ("lambdal", c_p), ("d_lambdal", c_p), ("temperature", ctypes.c_float)]


class GateMemberDesc(ctypes.Structure):
    """lbbnn_gate_member_desc_t"""
    _fields_ = [(n, c_p) for n in ("mu", "rho", "lambdal", "bias_mu", "bias_rho", "w_out", "bias_out", "gate_rows", "gates")] + \
               [(n, c_i) for n in ("O", "I", "ld", "flags", "exact")] + [("layer_id", c_u32)]


class FrozenDesc(ctypes.Structure):
    """lbbnn_frozen_desc_t"""
    _fields_ = [(n, c_p) for n in ("weight_mu", "weight_rho", "lambdal", "bias_rho", "q0_mean", "q0_log_var")] + \
               [("z_flow", PlanarFlow)] + \
               [(n, c_p) for n in ("e0", "e_w", "var_w", "bias_var", "kept_rows", "z_fwd", "e_w_members")] + \
               [("z_mstride", c_i64)] + [(n, c_i) for n in ("O", "I", "ld", "flags", "mode")] + \
               [("cut", ctypes.c_float), ("layer_id", c_u32)]


class CompactMap(ctypes.Structure):
    """lbbnn_compact_map_t"""
    _fields_ = [("rows", c_p), ("cols", c_p), ("O_full", c_i), ("I_full", c_i)]


class SparseDesc(ctypes.Structure):
    """lbbnn_sparse_desc_t"""
    _fields_ = [(n, c_p) for n in ("weight_mu", "weight_rho", "lambdal", "bias_rho", "row_ptr", "col", "mean", "var", "bias_var",
                                   "kept_rows")] + [("O", c_i), ("I", c_i), ("nnz", c_i), ("cut", ctypes.c_float)]


MAX_LEVELS = 16           # LBBNN_MAX_LEVELS: thresholds of one sweep


class SparseLevelsDesc(ctypes.Structure):
    """lbbnn_sparse_levels_desc_t"""
    _fields_ = [(n, c_p) for n in ("weight_mu", "weight_rho", "lambdal", "bias_rho", "row_ptr", "col", "mean", "var", "bias_var",
                                   "kept_rows")] + [("O", c_i), ("I", c_i), ("nnz", c_i), ("levels", c_i),
                                                    ("cut", ctypes.c_float * MAX_LEVELS)]


class SparseDrawDesc(ctypes.Structure):
    """lbbnn_sparse_draw_desc_t"""
    _fields_ = [(n, c_p) for n in ("col", "mean", "var", "bias_mu", "bias_var", "z")] + [("z_mstride", c_i64), ("tpos", c_p), ("wt", c_p), ("w", c_p),
               ("w_mstride", c_i64), ("b", c_p), ("b_mstride", c_i64), ("O", c_i), ("I", c_i), ("nnz", c_i), ("layer_id", c_u32)]


class SparseGatherArgs(ctypes.Structure):
    """lbbnn_sparse_gather_args_t"""
    _fields_ = [("ptr", c_p), ("idx", c_p), ("slot", c_p), ("w", c_p), ("w_mstride", c_i64), ("bias", c_p), ("b_mstride", c_i64),
                ("a", c_p), ("a_mstride", c_i64), ("h", c_p), ("h_mstride", c_i64), ("out", c_p), ("o_mstride", c_i64)] + \
               [(n, c_i) for n in ("lda", "ldh", "ldo", "B", "K", "N", "nnz", "mode", "relu", "out_rows", "a_shared", "blocks",
                                   "per_member")] + [("dot_bias", c_p), ("dot_b_mstride", c_i64), ("dot_acc", c_p)]


class MemberStatsArgs(ctypes.Structure):
    """lbbnn_member_stats_args_t"""
    _fields_ = [("t", c_p), ("t_mstride", c_i64)] + [(n, c_i) for n in ("ldt", "S", "C", "F", "B")] + \
               [(n, c_p) for n in ("mean", "std", "prob_pos", "prob_neg", "members", "logits")] + \
               [("ldl", c_i), ("n_logits", c_i), ("targets", c_p), ("intercept", c_p), ("residual", c_p)]


class BaseSparseDesc(ctypes.Structure):
    """lbbnn_base_sparse_desc_t"""
    _fields_ = [(n, c_p) for n in ("mu", "rho", "lambdal", "bias_mu", "bias_rho", "row_ptr", "col", "mean", "sigma", "b_mu",
                                   "b_sigma", "kept_rows")] + [("O", c_i), ("I", c_i), ("nnz", c_i)]


class BaseSparseDrawDesc(ctypes.Structure):
    """lbbnn_base_sparse_draw_desc_t"""
    _fields_ = [(n, c_p) for n in ("row_ptr", "col", "mean", "sigma", "b_mu", "b_sigma", "tpos", "wt", "w")] + \
               [("w_mstride", c_i64), ("b", c_p), ("b_mstride", c_i64), ("O", c_i), ("I", c_i), ("nnz", c_i), ("layer_id", c_u32)]


class BaseFrozenDesc(ctypes.Structure):
    """lbbnn_base_frozen_desc_t"""
    _fields_ = [(n, c_p) for n in ("mu", "rho", "lambdal", "bias_mu", "bias_rho", "w_mu", "w_sigma", "alpha", "e_w", "b_mu",
                                   "b_sigma", "kept_rows", "alpha_rows", "keep")] + \
               [(n, c_i) for n in ("O", "I", "ld", "flags", "exact")] + [("layer_id", c_u32)]


class DenseMembers(ctypes.Structure):
    """lbbnn_dense_members_t"""
    _fields_ = [("q0_mean", c_p), ("q0_log_var", c_p), ("zt", ctypes.POINTER(DenseTransform)), ("T", c_i), ("I", c_i),
                ("layer_id", c_u32), ("z_fwd", c_p), ("z_mstride", c_i64), ("mask_out", c_p)]


class OutGradArgs(ctypes.Structure):
    """lbbnn_outgrad_args_t"""
    _fields_ = [(n, c_p) for n in ("g_out", "out", "std", "eps", "rng", "gm", "gv", "gmT", "gvT", "g_sum", "gv_sum", "work")] + \
               [("row_offset", c_i64), ("rng_stream", c_u32)] + [(n, c_i) for n in ("B", "O", "ldg", "ldo", "relu")] + \
               [("gv_scale", c_p)]


class FlowStep(ctypes.Structure):
    """lbbnn_flow_step_t"""
    _fields_ = [("p0", c_p), ("p1", c_p), ("p2", c_p), ("type", c_i), ("M", c_i)]


class FlowChain(ctypes.Structure):
    """lbbnn_flow_chain_t"""
    _fields_ = [("step", FlowStep * MAX_FLOW_T), ("n", c_i)]


class PlanarGrad(ctypes.Structure):
    """lbbnn_planar_grad_t"""
    _fields_ = [("u", c_p * MAX_FLOW_T), ("w", c_p * MAX_FLOW_T), ("b", c_p * MAX_FLOW_T)]


class FlowBwdArgs(ctypes.Structure):
    """lbbnn_flow_bwd_args_t"""
    _fields_ = [(n, c_p) for n in ("q0_mean", "q0_log_var", "eps_fwd", "eps_kl", "r0_b1", "r0_b2", "aux",
                                   "dz_fwd", "dz_kl", "g_kl", "bias_mu", "bias_rho", "g_sum", "gv_sum")] + \
               [("z_flow", PlanarFlow), ("r_flow", PlanarFlow), ("priors", Priors)] + \
               [(n, c_p) for n in ("d_q0_mean", "d_q0_log_var", "d_r0_b1", "d_r0_b2", "d_bias_mu", "d_bias_rho")] + \
               [("d_z_flow", PlanarGrad), ("d_r_flow", PlanarGrad), ("work", c_p), ("O", c_i), ("I", c_i),
                ("rng", c_p), ("layer_id", c_u32)]


class DenseBwdArgs(ctypes.Structure):
    """lbbnn_dense_bwd_args_t"""
    _fields_ = [(n, c_p) for n in ("q0_mean", "q0_log_var", "eps_fwd", "eps_kl", "r0_b1", "r0_b2", "aux",
                                   "dz_fwd", "dz_kl", "g_kl", "bias_mu", "bias_rho", "g_sum", "gv_sum")] + \
               [("zt", ctypes.POINTER(DenseTransform)), ("rt", ctypes.POINTER(DenseTransform)),
                ("d_zt", ctypes.POINTER(DenseGrad)), ("d_rt", ctypes.POINTER(DenseGrad)), ("priors", Priors)] + \
               [(n, c_p) for n in ("d_q0_mean", "d_q0_log_var", "d_r0_b1", "d_r0_b2", "d_bias_mu", "d_bias_rho", "save", "work")] + \
               [("Tz", c_i), ("Tr", c_i), ("O", c_i), ("I", c_i), ("rng", c_p), ("layer_id", c_u32)]


EVAL_COUNTS = 6                        # LBBNN_EVAL_COUNTS, in the header's order:
EVAL_COUNT_NAMES = ("rows", "rows_with_target", "bad_targets", "correct_ensemble", "correct_posterior_mean",
                    "entropy_nonfinite")


class EvalMetricsArgs(ctypes.Structure):
    """lbbnn_eval_metrics_args_t"""
    _fields_ = [("logp", c_p), ("m_stride", c_i64), ("ldp", c_i64), ("mean_logp", c_p), ("ldm", c_i64), ("target", c_p),
                ("ens_logp", c_p), ("pred_ensemble", c_p), ("pred_mean", c_p), ("entropy", c_p),
                ("counts", c_p), ("correct_member", c_p), ("confusion", c_p), ("sums", c_p), ("work", c_p),
                ("S", c_i), ("B", c_i), ("C", c_i)]


MONITOR_COUNTS = 8                     # LBBNN_MONITOR_COUNTS, at the header's indices (LBBNN_MONITOR_STEPS ...):
MONITOR_COUNT_NAMES = ("steps", "rows", "correct", "bad_targets", "nonfinite_rows", "nonfinite_steps", "skipped_steps", "nll_rows")
MONITOR_SUMS = 5                       # LBBNN_MONITOR_SUMS, the doubles behind the counts:
MONITOR_SUM_NAMES = ("nll_sum", "kl_term_sum", "loss_sum", "last_nll", "last_loss")
MONITOR_WORDS = MONITOR_COUNTS + MONITOR_SUMS
MONITOR_SKIPPED_STEPS = 6              # LBBNN_MONITOR_SKIPPED_STEPS: the slot the guarded optimizer steps count in


UNC_COUNTS = 6                         # LBBNN_UNC_COUNTS, in the header's order:
UNC_COUNT_NAMES = ("rows", "rows_with_target", "bad_targets", "correct_bma", "nonfinite_rows", "log_score_nonfinite")
UNC_SUMS = 6                           # LBBNN_UNC_SUMS, in the header's order:
UNC_SUM_NAMES = ("total_entropy", "expected_entropy", "mutual_information", "confidence", "brier", "log_score")


class EvalUncertaintyArgs(ctypes.Structure):
    """lbbnn_eval_uncertainty_args_t"""
    _fields_ = [("logp", c_p), ("m_stride", c_i64), ("ldp", c_i64), ("target", c_p),
                ("bma_probs", c_p), ("pred_bma", c_p), ("confidence", c_p), ("total_entropy", c_p), ("expected_entropy", c_p),
                ("mutual_information", c_p), ("brier", c_p), ("log_score", c_p),
                ("counts", c_p), ("sums", c_p), ("bin_rows", c_p), ("bin_rows_with_target", c_p), ("bin_correct", c_p),
                ("bin_conf_sum", c_p), ("hist", c_p), ("work", c_p),
                ("S", c_i), ("B", c_i), ("C", c_i), ("conf_bins", c_i), ("hist_bins", c_i), ("ent_scale", ctypes.c_float)]


REG_COUNTS = 5                         # LBBNN_REG_COUNTS, in the header's order:
REG_COUNT_NAMES = ("elements", "elements_with_target", "bad_targets", "nonfinite_elements", "scored_elements")
REG_SUMS = 8                           # LBBNN_REG_SUMS, in the header's order:
REG_SUM_NAMES = ("sq_err", "abs_err", "log_density", "epistemic_var", "total_var", "y", "y2", "posterior_mean_sq_err")
REG_ROW_KEYS = ("pred_mean", "epistemic_var", "aleatoric_var", "total_std", "sq_err", "log_density", "pit")


class EvalRegressionArgs(ctypes.Structure):
    """lbbnn_eval_regression_args_t"""
    _fields_ = [("out", c_p), ("m_stride", c_i64), ("ldp", c_i64), ("mean_out", c_p), ("ldm", c_i64), ("target", c_p),
                ("ldt", c_i64), ("log_var", c_p)] + [(n, c_p) for n in REG_ROW_KEYS] + \
               [("counts", c_p), ("sums", c_p), ("pit_hist", c_p), ("work", c_p), ("S", c_i), ("B", c_i), ("O", c_i),
                ("pit_bins", c_i)]


SCORE_MAX_LEVELS = 4                   # LBBNN_SCORE_MAX_LEVELS
SCORE_MAX_MEMBERS = 64                 # LBBNN_SCORE_MAX_MEMBERS
SCORE_COUNTS = REG_COUNTS + SCORE_MAX_LEVELS           # LBBNN_SCORE_COUNTS: REG_COUNT_NAMES, then inside[level]
SCORE_SUMS = REG_SUMS + 2 + 2 * SCORE_MAX_LEVELS       # LBBNN_SCORE_SUMS: REG_SUM_NAMES, these two, width[level], interval_score[level]
SCORE_SUM_NAMES = REG_SUM_NAMES + ("aleatoric_var", "crps")
SCORE_ROW_KEYS = REG_ROW_KEYS + ("crps",)              # (B, units) each
SCORE_LEVEL_KEYS = ("lower", "upper", "interval_score")     # (levels, B, units) each


class EvalScoresArgs(ctypes.Structure):
    """lbbnn_eval_scores_args_t"""
    _fields_ = [("out", c_p), ("m_stride", c_i64), ("ldp", c_i64), ("mean_out", c_p), ("ldm", c_i64), ("target", c_p),
                ("ldt", c_i64), ("log_var", c_p), ("lv_mstride", c_i64), ("lv_ld", c_i64)] + \
               [(n, c_p) for n in SCORE_ROW_KEYS + SCORE_LEVEL_KEYS] + \
               [("counts", c_p), ("sums", c_p), ("pit_hist", c_p), ("work", c_p), ("S", c_i), ("B", c_i), ("O", c_i),
                ("pit_bins", c_i), ("n_levels", c_i), ("levels", ctypes.c_float * SCORE_MAX_LEVELS)]


STRUCTURE_MAX_LAYERS = 16             # LBBNN_STRUCTURE_MAX_LAYERS: layers per lbbnn_gate_structure call (= MAX_DEPTH)
STRUCTURE_MAX_WIDTH = 4096             # LBBNN_STRUCTURE_MAX_WIDTH: units per boundary


class StructureDesc(ctypes.Structure):
    """lbbnn_structure_desc_t"""
    _fields_ = [("lambdal", c_p), ("O", c_i), ("I", c_i), ("ld", c_i), ("layer_id", c_u32)]


EXPLAIN_SEED, EXPLAIN_MASK, EXPLAIN_FINISH = 0, 1, 2    # LBBNN_EXPLAIN_*: the modes of lbbnn_explain_step
GATHER_FORWARD, GATHER_SWEEP, GATHER_FINISH = 0, 1, 2   # LBBNN_GATHER_*: the post-ops of lbbnn_sparse_gather_members
MEMBER_BLOCKS_MAX = 65535              # members x explained outputs of one explain_ensemble call (gridDim.z)
EXPLAIN_MAX_OUTPUTS = 16               # LBBNN_EXPLAIN_MAX_OUTPUTS: rows of G per input row
EXPLAIN_MAX_ROWS = 1 << 24             # LBBNN_EXPLAIN_MAX_ROWS: B * C'


class ExplainStepArgs(ctypes.Structure):
    """lbbnn_explain_step_args_t"""
    _fields_ = [("mode", c_i), ("B", c_i), ("C", c_i), ("width", c_i), ("g", c_p), ("ldg", c_i64), ("w", c_p), ("ldw", c_i64),
                ("w_rows", c_i), ("targets", c_p), ("h", c_p), ("ldh", c_i64), ("bias", c_p), ("bias_out", c_p),
                ("intercept", c_p), ("active", c_p), ("ld_active", c_i64), ("mask_out", c_p), ("ldm", c_i64),
                ("logits", c_p), ("ldl", c_i64), ("map", c_p), ("full_width", c_i), ("contributions", c_p), ("ldc", c_i64),
                ("residual", c_p)]


# name -> (restype, argtypes); must list every symbol include/lbbnn.h declares
SIGNATURES = {
    "lbbnn_abi_version": (c_i, []),
    "lbbnn_error_string": (ctypes.c_char_p, [c_i]),
    "lbbnn_operand_ld": (c_i, [c_i]),
    "lbbnn_weight_pass": (c_i, [c_p, c_p, c_p, c_p, c_p, c_p, c_p, ctypes.POINTER(Priors),
                                c_p, c_p, c_i, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_p]),
    "lbbnn_weight_pass_f16": (c_i, [c_p, c_p, c_p, c_p, c_p, c_p, c_p, ctypes.POINTER(Priors),
                                    c_p, c_p, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_p]),
    "lbbnn_lrt_gemm_ex": (c_i, [ctypes.POINTER(GemmDesc), c_p]),
    "lbbnn_head_slab_floats": (c_i64, [c_i, c_i]),
    "lbbnn_format_x": (c_i, [c_p, c_i, c_p, c_i, c_i, c_i, c_p]),
    "lbbnn_lrt_gemm": (c_i, [c_p, c_i, c_p, c_p, c_i, c_p, c_p, c_p, c_p, c_p, c_u32, c_i64,
                             c_p, c_i, c_i, c_i, c_i, c_i, c_p]),
    "lbbnn_lrt_gemm_plan": (c_i, [c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, ctypes.POINTER(GemmPlan)]),
    "lbbnn_transpose_operand": (c_i, [c_p, c_i, c_i, c_i, c_p, c_i, c_i, c_i, c_p]),
    "lbbnn_weight_pass_backward_workspace": (c_i64, [c_i, c_i]),
    "lbbnn_weight_pass_backward": (c_i, [ctypes.POINTER(WpbArgs), c_p]),
    "lbbnn_layers_dense_flows": (c_i, [ctypes.POINTER(DenseLayer), c_i, c_p, c_p]),
    "lbbnn_layers_dense_flows_phase": (c_i, [ctypes.POINTER(DenseLayer), c_i, c_p, c_i, c_p]),
    "lbbnn_flow_dense_save_size": (c_i64, [c_i, c_i, c_i]),
    "lbbnn_mnf_flow_dense_backward_workspace": (c_i64, [c_i]),
    "lbbnn_mnf_flow_dense_backward": (c_i, [ctypes.POINTER(DenseBwdArgs), c_p]),
    "lbbnn_mnf_flow_dense_backward_batch": (c_i, [ctypes.POINTER(DenseBwdArgs), c_i, c_p]),
    "lbbnn_flow_dense_apply_workspace": (c_i64, [c_i, c_i]),
    "lbbnn_flow_dense_apply": (c_i, [ctypes.POINTER(DenseTransform), c_i, c_i, c_p, c_i, c_p, c_p, c_p]),
    "lbbnn_flow_dense_apply_backward": (c_i, [ctypes.POINTER(DenseTransform), ctypes.POINTER(DenseGrad), c_i, c_i, c_p, c_p,
                                              c_p, c_i, c_p, c_p, c_p]),
    "lbbnn_q0_rows": (c_i, [c_p, c_p, c_p, c_p, c_u32, c_i, c_i, c_p, c_p]),
    "lbbnn_flow_dense_rows_max_dim": (c_i, []),
    "lbbnn_flow_dense_rows": (c_i, [ctypes.POINTER(DenseTransform), c_i, c_p, c_p, c_p, c_u32, c_u64, c_p, c_i, c_i, c_i,
                                    c_p, c_i, c_p, c_p]),
    "lbbnn_gate_backward": (c_i, [ctypes.POINTER(GateBwdArgs), c_p, c_p]),
    "lbbnn_format_operand": (c_i, [c_p, c_i, c_i, c_i, c_p, c_i, c_i, c_i, c_p]),
    "lbbnn_multi_copy": (c_i, [ctypes.POINTER(CopyList), c_p]),
    "lbbnn_adam_step": (c_i, [ctypes.POINTER(AdamList), ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float,
                              ctypes.c_float, c_p, c_i, c_p]),
    "lbbnn_adam_step_groups": (c_i, [ctypes.POINTER(AdamGroupList), c_p, c_p, c_i, c_p, c_p, c_i, c_p]),
    "lbbnn_sgd_step_groups": (c_i, [ctypes.POINTER(AdamGroupList), c_p, c_p, c_i, c_p, c_p, c_i, c_p]),
    "lbbnn_adam_step_groups_guarded": (c_i, [ctypes.POINTER(AdamGroupList), c_p, c_p, c_i, c_p, c_p, c_i, c_p, c_p, c_p]),
    "lbbnn_sgd_step_groups_guarded": (c_i, [ctypes.POINTER(AdamGroupList), c_p, c_p, c_i, c_p, c_p, c_i, c_p, c_p, c_p]),
    "lbbnn_lrt_study_fit": (c_i, [ctypes.POINTER(StudyArgs), c_p]),
    "lbbnn_mnf_study_fit": (c_i, [ctypes.POINTER(MnfStudyArgs), c_p]),
    "lbbnn_grad_sumsq_workspace": (c_i64, [c_i64]),
    "lbbnn_grad_sumsq": (c_i, [ctypes.POINTER(AdamGroupList), c_p, c_i64, c_i64, ctypes.c_float, c_p, c_p, c_p]),
    "lbbnn_matmul_splitk": (c_i, [c_p, c_i, c_p, c_i, c_p, c_i, c_i, c_i, c_i, c_i, c_p]),
    "lbbnn_lrt_gemm_combine": (c_i, [c_p, c_i, c_p, c_i, c_p, c_i, c_p, c_i, c_p, c_i, c_i, c_i, c_i, c_i, c_p]),
    "lbbnn_dx_combine": (c_i, [c_p, c_p, c_p, c_i, c_i, c_i, c_p]),
    "lbbnn_output_grad_workspace": (c_i64, [c_i, c_i]),
    "lbbnn_output_grad": (c_i, [ctypes.POINTER(OutGradArgs), c_p]),
    "lbbnn_head_dx": (c_i, [c_p, c_p, c_i, c_p, c_p, c_i, c_p, c_i, c_p, c_i, c_i, c_i, c_i, c_p]),
    "lbbnn_head_dw": (c_i, [c_p, c_p, c_i, c_p, c_i, c_p, c_p, c_i, c_i, c_i, c_i, c_p]),
    "lbbnn_reduce_partials_batch": (c_i, [c_p, c_i, c_p]),
    "lbbnn_flow_chain": (c_i, [ctypes.POINTER(FlowChain), c_p, c_p, c_p, c_p, c_p, c_u32, c_i, c_p, c_p, c_p, c_p, c_p]),
    "lbbnn_flow_chain_rows": (c_i, [ctypes.POINTER(FlowChain), c_p, c_i, c_i, c_i, c_p, c_i, c_p, c_p]),
    "lbbnn_mnf_aux_backward": (c_i, [c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_p, c_p, c_p, c_p, c_u32, c_p]),
    "lbbnn_mnf_aux_backward_batch": (c_i, [c_p, c_i, c_p]),
    "lbbnn_bias_backward": (c_i, [c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_p]),
    "lbbnn_bias_backward_partials": (c_i, [c_p, c_i, c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p]),
    "lbbnn_mnf_flow_backward_workspace": (c_i64, [c_i, c_i, c_i]),
    "lbbnn_mnf_flow_planar_backward": (c_i, [ctypes.POINTER(FlowBwdArgs), c_p]),
    "lbbnn_mnf_flow_planar_backward_batch": (c_i, [ctypes.POINTER(FlowBwdArgs), c_i, c_p]),
    "lbbnn_mnf_flow_planar": (c_i, [c_p, c_p, c_p, c_p, c_p, c_i, c_p, c_p, c_p, c_i, c_p, c_p,
                                    c_p, c_u32, c_p, c_p, c_p, c_i, c_i, c_p]),
    "lbbnn_flow_dense_workspace": (c_i64, [c_i]),
    "lbbnn_mnf_flow_dense": (c_i, [c_p, c_p, ctypes.POINTER(DenseTransform), c_i, ctypes.POINTER(DenseTransform), c_i,
                                   c_p, c_p, c_p, c_u32, c_p, c_p, c_p, c_p, c_i, c_i, c_p]),
    "lbbnn_kl_finalize": (c_i, [c_p, c_p, c_p, c_i, c_p, c_p, c_p, c_p, c_p, c_i, c_p,
                                ctypes.POINTER(Priors), c_p, c_u32, c_p, c_p, c_i, c_p]),
    "lbbnn_flow_planar_form": (c_i, [c_i, c_p, c_p, c_p, c_p, c_p, c_i]),
    "lbbnn_kl_finalize_form": (c_i, [c_i, c_p, c_p, c_p, c_p, c_i]),
    "lbbnn_layers_prepare": (c_i, [ctypes.POINTER(LayerDesc), c_i, c_p, c_p]),
    "lbbnn_layers_operands_snap": (c_i, [ctypes.POINTER(LayerDesc), c_i, c_p, c_p, c_u64, c_p]),
    "lbbnn_layers_operands_x": (c_i, [ctypes.POINTER(LayerDesc), c_i, c_p, c_p, c_u64, c_p, c_i, c_p, c_i, c_i, c_i, c_p]),
    "lbbnn_ensemble_operands": (c_i, [ctypes.POINTER(LayerDesc), c_i, c_i, c_p, c_u64, c_p]),
    "lbbnn_lrt_gemm_members": (c_i, [c_p, c_i, c_i64, c_p, c_i64, c_p, c_i, c_p, c_p, c_p, c_u32, c_i64, c_u64,
                                     c_p, c_i, c_i64, c_i, c_i, c_i, c_i, c_i, c_p]),
    "lbbnn_layers_operands": (c_i, [ctypes.POINTER(LayerDesc), c_i, c_p, c_p]),
    "lbbnn_layers_finalize": (c_i, [ctypes.POINTER(LayerDesc), c_i, c_p, ctypes.c_uint64, c_p, c_p]),
    "lbbnn_kl_total": (c_i, [c_p, c_i, c_p, c_p]),
    "lbbnn_fold_rows": (c_i, [c_p, c_i, c_i, c_i, c_p, c_p]),
    "lbbnn_gate_sample": (c_i, [ctypes.POINTER(GateArgs), c_p, c_p]),
    "lbbnn_vd_operands": (c_i, [c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_p]),
    "lbbnn_weight_operands_t": (c_i, [c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_p]),
    "lbbnn_rng_advance": (c_i, [c_p, c_u64, c_p]),
    "lbbnn_philox_normal": (c_i, [c_p, c_u32, c_i64, c_i64, c_i64, c_p, c_p]),
    "lbbnn_gate_sample_draw": (c_i, [ctypes.POINTER(GateDrawArgs), c_p, c_p]),
    "lbbnn_gate_backward_draw": (c_i, [ctypes.POINTER(GateBwdDrawArgs), c_p, c_p]),
    "lbbnn_philox_uniform": (c_i, [c_p, c_u32, c_i64, c_i64, c_i64, c_p, c_p]),
    "lbbnn_gate_members": (c_i, [ctypes.POINTER(GateMemberDesc), c_i, c_i, c_i, ctypes.c_float, c_p, c_u64, c_p]),
    "lbbnn_gemm_members_mean": (c_i, [c_p, c_i, c_i64, c_p, c_i64, c_i, c_p, c_i64, c_p, c_i, c_i64, c_i, c_i, c_i, c_i, c_i,
                                      c_p]),
    "lbbnn_vd_gemm_members": (c_i, [c_p, c_i, c_i64, c_p, c_p, c_i, c_p, c_p, c_u32, c_i64, c_u64, c_p, c_i, c_i64,
                                    c_i, c_i, c_i, c_i, c_i, c_i, c_p]),
    "lbbnn_philox_std_gamma": (c_i, [c_p, c_u32, c_p, c_p, c_i64, c_p, c_p]),
    "lbbnn_gamma_grad": (c_i, [c_p, c_p, c_i64, c_p, c_p]),
    "lbbnn_elbo_loss": (c_i, [c_p, c_i, c_p, c_i, c_i, c_p, ctypes.c_float, c_p, c_p]),
    "lbbnn_elbo_loss_monitor": (c_i, [c_p, c_i, c_p, c_i, c_i, c_p, ctypes.c_float, c_p, c_p, c_p, c_p]),
    "lbbnn_elbo_loss_backward": (c_i, [c_p, c_p, c_i, c_i, ctypes.c_float, c_p, c_p, c_p]),
    "lbbnn_elbo_loss_backward_logits": (c_i, [c_p, c_p, c_p, c_i, c_i, c_i, ctypes.c_float, c_p, c_p, c_p, c_p]),
    "lbbnn_log_softmax_backward": (c_i, [c_p, c_i, c_p, c_i, c_p, c_i, c_i, c_i, c_p]),
    "lbbnn_log_softmax_rows": (c_i, [c_p, c_i, c_p, c_i, c_i, c_i, c_p]),
    "lbbnn_binary_head": (c_i, [c_p, c_i, c_i, c_i, c_p, c_i, c_p, c_i, c_p]),
    "lbbnn_elbo_bce_loss": (c_i, [c_p, c_i, c_p, c_i, c_i, c_i, c_p, ctypes.c_float, c_p, c_p, c_i, c_p]),
    "lbbnn_elbo_bce_loss_monitor": (c_i, [c_p, c_i, c_p, c_i, c_i, c_i, c_p, ctypes.c_float, c_p, c_p, c_i, c_p, c_p, c_p]),
    "lbbnn_elbo_bce_loss_backward": (c_i, [c_p, c_p, c_i, c_p, c_i, c_i, c_i, ctypes.c_float, c_p, c_p, c_p, c_p]),
    "lbbnn_sigmoid_backward": (c_i, [c_p, c_i, c_p, c_i, c_p, c_i, c_i, c_i, c_p]),
    "lbbnn_frozen_operands": (c_i, [ctypes.POINTER(FrozenDesc), c_i, c_p]),
    "lbbnn_frozen_members": (c_i, [ctypes.POINTER(FrozenDesc), c_i, c_i, c_p, c_u64, c_p]),
    "lbbnn_flow_dense_members_max_dim": (c_i, []),
    "lbbnn_flow_dense_members": (c_i, [ctypes.POINTER(DenseMembers), c_i, c_i, c_p, c_u64, c_p]),
    "lbbnn_frozen_members_dense": (c_i, [ctypes.POINTER(FrozenDesc), ctypes.POINTER(DenseMembers), c_i, c_i, c_p, c_u64, c_p]),
    "lbbnn_frozen_operands_compact": (c_i, [ctypes.POINTER(FrozenDesc), ctypes.POINTER(CompactMap), c_i, c_p]),
    "lbbnn_frozen_members_compact": (c_i, [ctypes.POINTER(FrozenDesc), ctypes.POINTER(CompactMap), c_i, c_i, c_p, c_u64, c_p]),
    "lbbnn_gather_columns": (c_i, [c_p, c_i, c_p, c_i, c_p, c_i, c_i, c_p]),
    "lbbnn_sparse_count": (c_i, [ctypes.POINTER(SparseDesc), c_i, c_p]),
    "lbbnn_sparse_pack": (c_i, [ctypes.POINTER(SparseDesc), c_i, c_p]),
    "lbbnn_frozen_members_z": (c_i, [ctypes.POINTER(FrozenDesc), c_i, c_i, c_p, c_u64, c_p]),
    "lbbnn_sparse_layer_members": (c_i, [c_p, c_p, c_p, c_p, c_i, c_p, c_p, c_p, c_i, c_i64, c_p, c_i64, c_p, c_u32, c_i64, c_u64,
                                         c_p, c_i, c_i64, c_i, c_i, c_i, c_i, c_i, c_i, c_p]),
    "lbbnn_sparse_count_levels": (c_i, [ctypes.POINTER(SparseLevelsDesc), c_i, c_p]),
    "lbbnn_sparse_pack_levels": (c_i, [ctypes.POINTER(SparseLevelsDesc), c_i, c_p]),
    "lbbnn_sparse_layer_levels": (c_i, [c_p, c_p, c_p, c_p, c_i, c_p, c_p, c_p, c_i, c_i64, c_p, c_i64, c_p, c_u32, c_i64, c_u64,
                                        c_p, c_i, c_i64, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_p]),
    "lbbnn_base_frozen_operands": (c_i, [ctypes.POINTER(BaseFrozenDesc), ctypes.POINTER(CompactMap), c_i, c_i, ctypes.c_float, c_p]),
    "lbbnn_base_frozen_members": (c_i, [ctypes.POINTER(BaseFrozenDesc), ctypes.POINTER(CompactMap), c_i, c_i, c_i, ctypes.c_float,
                                        ctypes.POINTER(c_p), ctypes.POINTER(c_p), ctypes.POINTER(c_p), c_p, c_u64, c_p]),
    "lbbnn_eval_metrics_work_bytes": (c_i64, [c_i, c_i, c_i]),
    "lbbnn_eval_metrics": (c_i, [ctypes.POINTER(EvalMetricsArgs), c_p]),
    "lbbnn_eval_uncertainty_work_bytes": (c_i64, [c_i, c_i, c_i, c_i]),
    "lbbnn_eval_uncertainty": (c_i, [ctypes.POINTER(EvalUncertaintyArgs), c_p]),
    "lbbnn_eval_regression_work_bytes": (c_i64, [c_i, c_i, c_i]),
    "lbbnn_eval_regression": (c_i, [ctypes.POINTER(EvalRegressionArgs), c_p]),
    "lbbnn_eval_regression_scores_work_bytes": (c_i64, [c_i, c_i, c_i, c_i]),
    "lbbnn_eval_regression_scores": (c_i, [ctypes.POINTER(EvalScoresArgs), c_p]),
    "lbbnn_elbo_gaussian_loss": (c_i, [c_p, c_i, c_p, c_i, c_p, c_i, c_i, c_i, c_p, ctypes.c_float, c_p, c_p, c_p, c_p]),
    "lbbnn_elbo_gaussian_loss_monitor": (c_i, [c_p, c_i, c_p, c_i, c_p, c_i, c_i, c_i, c_p, ctypes.c_float, c_p, c_p, c_p, c_p, c_p,
                                               c_p]),
    "lbbnn_elbo_gaussian_loss_backward": (c_i, [c_p, c_p, c_i, c_p, c_i, c_p, c_i, c_i, c_i, ctypes.c_float, c_p, c_p, c_p, c_p,
                                                c_p]),
    "lbbnn_gate_structure_width": (c_i64, [ctypes.POINTER(StructureDesc), c_i]),
    "lbbnn_gate_structure": (c_i, [ctypes.POINTER(StructureDesc), c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p]),
    "lbbnn_explain_step": (c_i, [ctypes.POINTER(ExplainStepArgs), c_p]),
    "lbbnn_explain_work_bytes": (c_i64, [c_i, c_i, c_i]),
    "lbbnn_explain_totals": (c_i, [c_p, c_i64, c_p, c_i, c_i, c_i, c_p, c_p, c_p, c_p, c_p]),
    "lbbnn_explain_operand": (c_i, [c_p, c_i, c_i, c_i, c_p, c_p]),
    "lbbnn_sparse_draw_members": (c_i, [ctypes.POINTER(SparseDrawDesc), c_i, c_i, c_p, c_i, c_p]),
    "lbbnn_sparse_gather_members": (c_i, [ctypes.POINTER(SparseGatherArgs), c_p]),
    "lbbnn_explain_seed": (c_i, [c_p, c_p, c_i, c_p, c_p, c_i64, c_p, c_i, c_p, c_i, c_i, c_i, c_i, c_p, c_u64, c_p]),
    "lbbnn_explain_member_stats": (c_i, [ctypes.POINTER(MemberStatsArgs), c_p]),
    "lbbnn_base_sparse_count": (c_i, [ctypes.POINTER(BaseSparseDesc), c_i, ctypes.c_float, c_p]),
    "lbbnn_base_sparse_pack": (c_i, [ctypes.POINTER(BaseSparseDesc), c_i, ctypes.c_float, c_p]),
    "lbbnn_base_sparse_draw_members": (c_i, [ctypes.POINTER(BaseSparseDrawDesc), c_i, c_i, c_p, c_u64, c_i, c_p]),
}

_lib = None


def lib():
    """Load (once) and return the shared library; raise loudly if it is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "bnn_amd: HIP extension not built: %s is missing. Build it with "
                "`python -c 'import __graft_entry__ as g; g.build()'` or "
                "`make -C bayesian-neural-nets_amd/csrc` (hipcc, --offload-arch=gfx950). "
                "There is no CPU fallback." % LIB_PATH)
        l = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(l, name)      # AttributeError => header/library out of sync: fail loudly
            fn.restype = res
            fn.argtypes = args
        _lib = l
    if RECORD is not None:
        return _Recorder(_lib)
    return _lib


# graphs.LaunchPlan: while RECORD is a list, every C call made through lib() is appended to it as (function, arguments) -- the
# arguments are what ctypes was given (ints, None, ctypes arrays / structs: the latter stay alive with the record)
RECORD = None


class _Recorder:
    def __init__(self, l):
        self._l = l

    def __getattr__(self, name):
        fn = getattr(self._l, name)

        def call(*args):
            # only what ENQUEUES is recorded: every such entry point ends in `void* stream`; the size / version helpers do not
            if RECORD is not None and fn.argtypes and fn.argtypes[-1] is ctypes.c_void_p:
                RECORD.append((name, fn, args))
            return fn(*args)
        return call


def check(rc, what):
    if rc != 0:
        msg = lib().lbbnn_error_string(rc)
        raise RuntimeError("bnn_amd: %s failed (%d): %s" % (what, rc, msg.decode() if msg else "?"))


def launch(dev, name: str, *args):
    """One library call on ``dev``'s current stream (its last argument), checked."""
    import torch
    check(getattr(lib(), name)(*args, torch.cuda.current_stream(dev).cuda_stream), name)
