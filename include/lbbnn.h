/*
 * lbbnn.h -- C ABI of the MI355X (gfx950) Bayesian linear-layer hot path.
 *
 * Drop-in boundary for LarsELund/Bayesian-Neural-Nets' BayesianLinear.forward family.
 * The reference has no native layer: its "FFI" is the set of PyTorch aten calls the layer
 * issues.  Each entry point below replaces one group of those calls and
 * cites the reference lines it stands for (paths relative to the reference checkout).
 *
 * Conventions
 *  - Every pointer is a DEVICE pointer to contiguous row-major fp32 unless stated otherwise.
 *    The caller (PyTorch) owns all buffers, including workspaces; nothing here allocates.
 *  - `stream` is a hipStream_t passed as void*.  Calls only enqueue work and return; they
 *    never synchronise and are safe under HIP-graph capture.  The only process-wide state is an idempotent cache
 *    of "dynamic-LDS limit already raised" per kernel (hipFuncSetAttribute is a host-side attribute, not a stream
 *    operation); a few environment variables read once select measurement knobs (LBBNN_GEMM_RESIDENCY, LBBNN_GEMM_NO_DMA).
 *  - Return value: 0 on success; a negative LBBNN_E_* for argument errors (nothing was
 *    launched); a positive hipError_t if the launch failed.  No C++ exception crosses.
 *  - Noise: every stochastic entry takes either an explicit draw (`eps`, parity mode) or,
 *    when that pointer is NULL, generates N(0,1) in-kernel with Philox4x32-10 keyed by the
 *    two 64-bit words at `rng` = {seed, offset} (device memory, so a captured graph sees
 *    fresh noise on every replay after lbbnn_rng_advance).
 */
#ifndef LBBNN_H_
#define LBBNN_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LBBNN_ABI_VERSION 1

#define LBBNN_OK 0
#define LBBNN_E_NULL (-1)      /* a required pointer is NULL                    */
#define LBBNN_E_SHAPE (-2)     /* a dimension is <= 0 or exceeds a kernel limit */
#define LBBNN_E_ALIGN (-3)     /* a pointer / leading dimension is misaligned   */
#define LBBNN_E_FLAGS (-4)     /* unknown or inconsistent flag bits             */
#define LBBNN_E_NOISE (-5)     /* neither an explicit draw nor an rng state     */

#define LBBNN_MAX_FLOW_T 16    /* max transforms per planar flow ('mixed' uses 10)  */
#define LBBNN_MAX_FLOW_DIM 16384

/* GEMM flags */
#define LBBNN_F_RELU 0x1       /* fuse F.relu on the output (LBBNN-GP-MF-LRT.py:208-209)      */
#define LBBNN_F_MEAN_ONLY 0x2  /* posterior-mean branch: out = x.e_w^T + b (…LRT.py:178-180)  */
#define LBBNN_F_SPLIT16 0x4    /* split-precision MFMA path: bf16x3 products, operands hi + lo  */
#define LBBNN_F_LOG_SOFTMAX 0x8 /* fuse F.log_softmax(dim=1) on the output; O <= 16 only (…LRT.py:210) */
#define LBBNN_F_HALF16 0x20    /* with LBBNN_F_SPLIT16 | LBBNN_F_SINGLE16: the single product in FP16 (v_mfma_f32_16x16x32_f16; operands
                                  from lbbnn_vd_operands(LBBNN_F_HALF16): fp16 in the hi units) -- the "fp16 MFMA" of BASELINE
                                  configs[4]; unscaled, so only for operands inside fp16's range (the variational-dropout theta) */
#define LBBNN_F_SINGLE16 0x10  /* with LBBNN_F_SPLIT16, lbbnn_lrt_gemm only: ONE bf16 product per moment (the hi parts of the
                                  same operands, x rounded to bf16 in registers) -- the plain "bf16 MFMA" arithmetic that
                                  BASELINE configs[1] names; 2e-3 relative on the mean GEMM, outside the 1e-4 contract */

/* Philox stream ids (third counter word) -- one per kind of draw, per layer (stream = kind*64+layer) */
#define LBBNN_STREAM_EPS_OUT 0
#define LBBNN_STREAM_EPS_Z 1
#define LBBNN_STREAM_EPS_Z2 2
#define LBBNN_STREAM_EPS_ACT 3
#define LBBNN_STREAM_MASK 6    /* Bernoulli(0.5) masks of the dense flows (lbbnn_dense_layer_t::draw_masks) */
#define LBBNN_STREAM_ROW_MASK 7 /* per-row masks of lbbnn_flow_dense_rows (stream id = 7*64 + layer id by convention)  */

/* Prior constants of one layer.  The reference keeps them as constant tensors:
 * LBBNN-GP-MF-LRT.py:142-143,151,159-160; LBBNN-GP-MF-MNF.py:145-146,154,162-163. */
typedef struct lbbnn_priors {
    float mu_prior;          /* 0    */
    float sigma_prior;       /* 1    */
    float alpha_prior;       /* 0.05 */
    float bias_mu_prior;     /* 0    */
    float bias_sigma_prior;  /* 1    */
} lbbnn_priors_t;

int lbbnn_abi_version(void);
const char* lbbnn_error_string(int code);

/* Round a K extent up to the operand leading dimension the GEMM expects (multiple of 32). */
int lbbnn_operand_ld(int I);

/* ---------------------------------------------------------------------------------------------
 * K1  lbbnn_weight_pass -- one fused, coalesced pass over the (O,I) variational parameters.
 *
 * Replaces, per layer and per forward:
 *   alpha = 1/(1+exp(-lambdal))                       LBBNN-GP-MF-LRT.py:167, …MNF.py:191
 *   sigma = log1p(exp(rho))  (recomputed 3-4x there)  …LRT.py:81-82
 *   e_w = mu*alpha ; var_w = sigma^2*alpha^2           …LRT.py:170-171, …MNF.py:195-196
 *   kl_weight integrand + row sums                     …LRT.py:189-192, …MNF.py:230-233
 *   act_mu = r0_c @ (z2*mu*alpha)^T, act_var = r0_c^2 @ var_w^T     …MNF.py:211-212,216-217
 *   bias sigma^2                                       …LRT.py:173
 *
 * Inputs : mu, rho, lambdal (O,I).  z_fwd (I) or NULL: per-input multiplier z_k folded into
 *          the mean operand (…MNF.py:197).  z_kl (I) or NULL: z2 of the KL branch (…MNF.py:210).
 *          r0_c (I) or NULL.  bias_rho (O) or NULL.
 * Outputs: e_w, var_w: GEMM operands [O][ld] (ld = lbbnn_operand_ld(I), zero-filled tail),
 *          either may be NULL.  kl_rows (O): per-row sum of the KL integrand (NULL = skip).
 *          act_mu, act_var (O) (NULL = skip; need z_kl and r0_c).  bias_var (O) = softplus(bias_rho)^2.
 *          With LBBNN_F_SPLIT16 each operand row (the same 4*ld bytes) holds w = hi + lo in bf16: per 32-k chunk one
 *          128-B line of 16-B units, unit 2g = hi of k in [8g, 8g+8), unit 2g+1 = lo of the same k; see DESIGN.md
 *          "Data layout".  The format is produced and consumed only by this library.
 */
int lbbnn_weight_pass(const float* mu, const float* rho, const float* lambdal,
                      const float* z_fwd, const float* z_kl, const float* r0_c,
                      const float* bias_rho, const lbbnn_priors_t* priors,
                      void* e_w, void* var_w, int ld,
                      float* kl_rows, float* act_mu, float* act_var, float* bias_var,
                      int O, int I, int flags, void* stream);

/* ---------------------------------------------------------------------------------------------
 * K2  lbbnn_lrt_gemm -- the two activation-moment GEMMs + local-reparameterisation epilogue.
 *
 *   mean = x . e_w^T + bias_mean          torch.mm  …LRT.py:172, …MNF.py:197
 *   var  = x^2 . var_w^T (* var_scale) + bias_var      …LRT.py:173, …MNF.py:198  (x^2 formed in registers)
 *   out  = mean + sqrt(var) * eps         randn + sample  …LRT.py:174-175, …MNF.py:199-200
 *   optional ReLU                         …LRT.py:208-209
 * LBBNN_F_MEAN_ONLY: out = mean (…LRT.py:178-180; F.linear of LBBNN-GP-MF.py:255).
 *
 * x (B,I) with row stride ldx floats; e_w/var_w operands from lbbnn_weight_pass (leading dim ld);
 * bias_mean/bias_var/var_scale (O) or NULL (0 / 0 / 1); eps (B,O) or NULL => Philox from `rng`
 * with counter = (row_offset + b, o/4), stream id `rng_stream`; out (B,O) row stride ldo.
  * B == 0 (empty batch) is a successful no-op.
 */
int lbbnn_lrt_gemm(const float* x, int ldx, const void* e_w, const void* var_w, int ld,
                   const float* bias_mean, const float* bias_var, const float* var_scale,
                   const float* eps, const uint64_t* rng, uint32_t rng_stream, int64_t row_offset,
                   float* out, int ldo, int B, int I, int O, int flags, void* stream);

/* lbbnn_lrt_gemm_plan -- which kernel instantiation lbbnn_lrt_gemm and its member / fan-out / combine / split-K forms launch
 * for a call, answered on the host: no pointer is taken, no GPU is touched.  It is the selection function the dispatcher
 * itself launches from, so the answer cannot drift from what runs.
 *   family      LBBNN_GEMM_SKINNY (O <= 16) | LBBNN_GEMM_STAGED (fp32, register-staged) | LBBNN_GEMM_DMA (fp32, LDS-DMA)
 *               | LBBNN_GEMM_SPLIT (16-bit operands, LBBNN_F_SPLIT16); LBBNN_GEMM_NONE for B == 0 (nothing is launched)
 *   large_tile  1: the 80 x 128 tile (four waves), 0: 80 x 32 (two waves); 0 for the skinny kernel
 *   xvec        x rows are read as 16-B vectors (always 1 for the DMA and split families)
 *   mean_only   the mean product alone, no noise
 *   products    matrix products per moment: 3 or 1 for the split family (LBBNN_F_SINGLE16 on a dual launch), else 1
 *   half        the single product in fp16 (LBBNN_F_HALF16)
 *   fan         the fan-out form of lbbnn_vd_gemm_members (one tile product, every member's epilogue)
 *   kernel_id   one integer per instantiation: equal ids, same kernel
 * Inputs: the call's B, I, O, ldx; x_aligned: x sits on a 16-B boundary; flags as for lbbnn_lrt_gemm; members (>= 1, > 1: the
 * member forms); fan (> 0: fan-out over that many members); kchunk (> 0: lbbnn_matmul_splitk's chunk).  Returns 0, or the
 * code the launch would return for these inputs (LBBNN_E_SHAPE / _FLAGS / _ALIGN); checks that need a pointer or the operand
 * stride ld stay with the launch.  Whether the KL finalize rides in the launch depends on LDS and is not part of the plan.
 * The environment knob LBBNN_GEMM_NO_DMA (read once) turns the DMA family into the staged one here as in the launch. */
#define LBBNN_GEMM_NONE (-1)
#define LBBNN_GEMM_SKINNY 0
#define LBBNN_GEMM_STAGED 1
#define LBBNN_GEMM_DMA 2
#define LBBNN_GEMM_SPLIT 3
typedef struct lbbnn_gemm_plan {
    int family, large_tile, xvec, mean_only, products, half, fan, kernel_id;
} lbbnn_gemm_plan_t;
int lbbnn_lrt_gemm_plan(int B, int I, int O, int ldx, int x_aligned, int flags, int members, int fan, int kchunk,
                        lbbnn_gemm_plan_t* plan);

/* ---------------------------------------------------------------------------------------------
 * K3  lbbnn_mnf_flow_planar -- z sampling + planar flows of one MNF layer, one launch.
 *
 * Replaces sample_z (LBBNN-GP-MF-MNF.py:182-187) called twice per training forward, the planar
 * transforms (flows2.py:86-95, PropagateFlow.forward :41-46), log_q0 (…MNF.py:213-214) and
 * r_flow(z2) (…MNF.py:222).  Only the row the reference keeps (zs[-1], quirk 1 of SURVEY.md 3.2)
 * is computed.
 *
 *   z_fwd = z_flow(q0_mean + exp(q0_log_var)^.5 * eps_fwd)            (forward multiplier z_k)
 *   z0    = q0_mean + exp(q0_log_var)^.5 * eps_kl ; z_kl = z_flow(z0) (KL branch z2)
 *   scal[0] = log_det_q   scal[1] = log_q0 (uses -0.5*log(pi), quirk 3)
 *   scal[2] = log_det_r   scal[3] = r_flow(z_kl)[-1]  (last ELEMENT, quirk 2)
 *   scal[4] = log-det of the forward draw's z_flow (what sample_z(B) returns next to z_k)
 *
 * zu/zw/zb (ru/rw/rb): host arrays of T device pointers to the u (I), w (I), bias (1) of each
 * transform.  eps_fwd / eps_kl: (I) draws or NULL => Philox (streams EPS_Z / EPS_Z2, counter = i/4).
 * want_kl == 0 computes z_fwd (and scal[4] if scal != NULL) only.  z_fwd / z_kl (I) outputs; scal: 8 floats.
 */
int lbbnn_mnf_flow_planar(const float* q0_mean, const float* q0_log_var,
                          const float* const* zu, const float* const* zw, const float* const* zb, int Tz,
                          const float* const* ru, const float* const* rw, const float* const* rb, int Tr,
                          const float* eps_fwd, const float* eps_kl,
                          const uint64_t* rng, uint32_t layer_id,
                          float* z_fwd, float* z_kl, float* scal,
                          int I, int want_kl, void* stream);


/* ---------------------------------------------------------------------------------------------
 * K4  lbbnn_mnf_flow_dense -- z sampling + dense coupling flows (RNVP / MNF type) of one MNF layer.
 *
 * Same outputs as lbbnn_mnf_flow_planar (z_fwd, z_kl, scal[0..4]) for the reference's default flow
 * types: RNVP (flows2.py:188-219: mask, 4-layer LeakyReLU(0.1) MLP I->75->75->75->75, t/s heads,
 * sigmoid gate, Sum (1-m) log gate) and MNF (flows2.py:225-241: mask, tanh(f(m z)) 100 hidden units,
 * g/k heads, Sum (1-m) log sigma).  Only the kept row (zs[-1]) is computed, so every dense step is a
 * GEMV; per transform: one launch spreads the I-long dot products of the hidden units over
 * workgroups, one launch produces the I outputs (recomputing the tiny H x H chain per workgroup) and
 * per-workgroup log-det partials that are summed in a fixed order (deterministic).
 *
 * Bernoulli(0.5) masks (flows2.py:209,234) are explicit inputs (the host wrapper draws them):
 * mask_fwd = the forward draw's z_flow call, mask_kl = the KL branch's z_flow / r_flow call.
 * work: caller-owned scratch of lbbnn_flow_dense_workspace(I) floats.
 */
#define LBBNN_FLOW_RNVP 0
#define LBBNN_FLOW_MNF 1
#define LBBNN_MAX_HIDDEN 128

typedef struct lbbnn_dense_transform {
    int kind;                               /* LBBNN_FLOW_RNVP / LBBNN_FLOW_MNF                         */
    int hidden;                             /* 75 (RNVP) / 100 (MNF); <= LBBNN_MAX_HIDDEN               */
    const float *w_in, *b_in;               /* (H,I),(H): RNVP network.0 | MNF f                        */
    const float *w_mid[3], *b_mid[3];       /* (H,H),(H): RNVP network.2/4/6 | NULL for MNF             */
    const float *w_a, *b_a;                 /* (I,H),(I): RNVP t (shift) | MNF g (mu)                   */
    const float *w_b, *b_b;                 /* (I,H),(I): RNVP s (scale) | MNF k (sigma pre-activation) */
    const float *mask_fwd, *mask_kl;        /* (I) each, values in {0,1}                                */
} lbbnn_dense_transform_t;

int64_t lbbnn_flow_dense_workspace(int I);

int lbbnn_mnf_flow_dense(const float* q0_mean, const float* q0_log_var,
                         const lbbnn_dense_transform_t* zt, int Tz,
                         const lbbnn_dense_transform_t* rt, int Tr,
                         const float* eps_fwd, const float* eps_kl,
                         const uint64_t* rng, uint32_t layer_id,
                         float* z_fwd, float* z_kl, float* scal, float* work,
                         int I, int want_kl, void* stream);

/* The same for up to LBBNN_MAX_LAYERS layers at once (blockIdx.z = layer): 2 + 2*(Tz+Tr) launches for the whole network
 * instead of that many per layer.  The layers must agree on Tz, Tr and want_kl (LBBNN_E_SHAPE otherwise). */
typedef struct lbbnn_dense_layer {
    const float *q0_mean, *q0_log_var;
    const lbbnn_dense_transform_t *zt, *rt;
    const float *eps_fwd, *eps_kl;
    float *z_fwd, *z_kl, *scal, *work;          /* work: lbbnn_flow_dense_workspace(I) floats */
    int Tz, Tr, I, want_kl;
    uint32_t layer_id;
    float *save;                                 /* NULL, or lbbnn_flow_dense_save_size(I, Tz, Tr) floats: the forward keeps the
                                                    input of every transform and the hidden activations of the coupling MLPs
                                                    there for lbbnn_mnf_flow_dense_backward */
    int draw_masks;                              /* 1: the mask vectors of zt / rt are OUTPUTS of this call -- Bernoulli(0.5)
                                                    (flows2.py:209,234) from Philox stream LBBNN_STREAM_MASK of `rng`
                                                    (required), counter = row i: bit t of word 0 / 1 / 2 = transform t of the
                                                    z flow's forward call / its KL call / the r flow -- written by the first
                                                    launch; 0: they are inputs */
} lbbnn_dense_layer_t;

int64_t lbbnn_flow_dense_save_size(int I, int Tz, int Tr);
int lbbnn_layers_dense_flows(const lbbnn_dense_layer_t* layers, int n, const uint64_t* rng, void* stream);
/* The same launches in two parts, so that the part only the KL needs can leave the critical path of a forward
 * (LBBNN-GP-MF-MNF.py:190-200 needs z_k only; :208-235 need the rest): phase 1 = the draws and the z flow on both draws
 * (outputs z_fwd, z_kl), phase 2 = the r flow on the KL draw and the scalars (scal); phase 0 = both (the call above).
 * Phase 2 must follow phase 1 of the same call arguments (it continues in `work`); it may be enqueued on another stream
 * once phase 1 has completed there. */
int lbbnn_layers_dense_flows_phase(const lbbnn_dense_layer_t* layers, int n, const uint64_t* rng, int phase, void* stream);

/* ---------------------------------------------------------------------------------------------
 * K5  lbbnn_kl_finalize -- the O(O+I) tail of the KL and the final scalar.
 *
 *   kl_bias                                                    …LRT.py:185-186, …MNF.py:227-228
 *   act = tanh(act_mu + sqrt(act_var)*eps_act); mean_r, log_var_r; log_rb   …MNF.py:218-224
 *   kl = kl_bias + sum(kl_rows) + (-log_det_q + log_q0) - (log_det_r + log_rb)   …MNF.py:215,225,235
 * LRT (scal == NULL): kl = kl_bias + sum(kl_rows)               …LRT.py:194
 *
 * kl_accum: if nonzero, *kl_out += kl (BayesianNetwork.kl(), …LRT.py:213-214), else *kl_out = kl.
 */
int lbbnn_kl_finalize(const float* kl_rows, const float* bias_mu, const float* bias_rho, int O,
                      const float* act_mu, const float* act_var, const float* eps_act,
                      const float* r0_b1, const float* r0_b2, int I,
                      const float* scal, const lbbnn_priors_t* priors,
                      const uint64_t* rng, uint32_t layer_id,
                      float* kl_out, float* kl_layer, int kl_accum, void* stream);

/* lbbnn_flow_planar_form / lbbnn_kl_finalize_form -- which kernel form a K3 / K5 launch takes, answered on the host: no
 * device pointer is taken, no GPU is touched.  Each is the selection function the launcher itself launches from, so the answer
 * cannot drift from what runs.  The per-layer arrays are HOST arrays of n entries, 1 <= n <= LBBNN_MAX_LAYERS.
 *
 * lbbnn_flow_planar_form: the form of ONE K3 launch over n layers (lbbnn_mnf_flow_planar: n = 1; lbbnn_layers_prepare /
 *   _operands: the MNF layers of the call without flows_done; lbbnn_ensemble_operands: members > 1).  I, Tz, Tr, want_kl as
 *   in the layer (Tr is ignored without want_kl); aligned16[i] != 0: every vector of layer i the launch touches (q0_mean,
 *   q0_log_var, z_fwd, the explicit draws, z_kl with want_kl, u and w of every transform) sits on a 16-B boundary and the
 *   member stride of z_fwd is a multiple of 4.  Returns
 *     LBBNN_K3_GENERIC  vectors read from global memory, z in LDS (the largest layer is past the 144 KiB LDS budget)
 *     LBBNN_K3_LDS      inputs staged in LDS, one reduction per transform (a layer with more than 4 transforms)
 *     LBBNN_K3_FAST     inputs staged in LDS, one reduction for the whole chain
 *     LBBNN_K3_VEC      the same chain in registers (every layer: I % 4 == 0, I <= 2048, aligned16)
 *   or the code the launch would return: NULL array: LBBNN_E_NULL; n, members (1 .. 65535), I (1 .. LBBNN_MAX_FLOW_DIM), Tz
 *   or Tr (0 .. LBBNN_MAX_FLOW_T) out of range, members > 1 where the launch is neither FAST nor VEC: LBBNN_E_SHAPE.  The
 *   environment knob LBBNN_K3_VEC=0 (read once) turns VEC into FAST here as in the launch.
 *
 * lbbnn_kl_finalize_form: all_layers == 0: the per-layer launch of lbbnn_kl_finalize (n = 1) and lbbnn_layers_prepare (its
 *   layers with want_kl; active is ignored and may be NULL): LBBNN_K5_LDS if the LARGEST layer's vectors fit the budget, else
 *   LBBNN_K5_GENERIC.  all_layers != 0: the single-workgroup launch of lbbnn_layers_finalize: LBBNN_K5_STAGED if the vectors
 *   of all ACTIVE layers (want_kl) fit together, else LBBNN_K5_UNSTAGED.  mnf[i] != 0: the layer has the auxiliary terms
 *   (scal != NULL); I is read for those layers only.  NULL array: LBBNN_E_NULL; n out of range, O < 1 or I < 1 of a layer that
 *   is read: LBBNN_E_SHAPE. */
#define LBBNN_K3_GENERIC 0
#define LBBNN_K3_LDS 1
#define LBBNN_K3_FAST 2
#define LBBNN_K3_VEC 3
#define LBBNN_K5_GENERIC 0
#define LBBNN_K5_LDS 1
#define LBBNN_K5_UNSTAGED 0
#define LBBNN_K5_STAGED 1
int lbbnn_flow_planar_form(int n, const int* I, const int* Tz, const int* Tr, const int* want_kl, const int* aligned16,
                           int members);
int lbbnn_kl_finalize_form(int n, const int* O, const int* I, const int* mnf, const int* active, int all_layers);


/* ---------------------------------------------------------------------------------------------
 * Batched "prepare": everything in a network forward that does NOT depend on the activations
 * (K3 flows, K1 weight pass, K5 KL finalize) for up to LBBNN_MAX_LAYERS layers in three launches
 * on one stream -- one launch per kernel kind covering all layers -- so the critical path of
 * BayesianNetwork.forward (LBBNN-GP-MF-MNF.py:252-257) is  prepare -> GEMM1 -> GEMM2 -> GEMM3.
 * Field meaning = the arguments of the single-layer entry points above.
 */
#define LBBNN_MAX_LAYERS 4

typedef struct lbbnn_planar_flow {
    const float* u[LBBNN_MAX_FLOW_T];
    const float* w[LBBNN_MAX_FLOW_T];
    const float* b[LBBNN_MAX_FLOW_T];
    int T;
} lbbnn_planar_flow_t;

typedef struct lbbnn_layer_desc {
    /* parameters (state_dict names of the reference) */
    const float *weight_mu, *weight_rho, *lambdal, *bias_mu, *bias_rho;
    const float *q0_mean, *q0_log_var, *r0_c, *r0_b1, *r0_b2;      /* all NULL for an LRT layer */
    lbbnn_planar_flow_t z_flow, r_flow;
    lbbnn_priors_t priors;
    int O, I;
    uint32_t layer_id;
    int stochastic;          /* produce var_w (training or sample)            */
    int want_kl;             /* training or calculate_log_probs               */
    int split;               /* operand format: 0 fp32; 1 bf16 hi + lo (LBBNN_F_SPLIT16); 2 fp16 hi + lo with per-row power-of-two
                                scales (LBBNN_F_F16S: needs e_scale / v_scale below, rows of at most 1280 weights); 3 the same
                                for e_w and var_w as plain fp16 rows, hi part only (the operands of LBBNN_F_F16S | LBBNN_F_VAR1) */
    /* explicit draws; NULL => Philox from rng */
    const float *eps_z, *eps_z2, *eps_act;
    /* caller-owned workspace */
    float *z_fwd, *z_kl, *scal;                  /* (I), (I), 8 floats; MNF only */
    void *e_w, *var_w;                           /* [O][lbbnn_operand_ld(I)]     */
    float *kl_rows, *act_mu, *act_var, *bias_var;/* (O) each                     */
    float* kl_layer;                             /* 1 float: this layer's KL     */
    int flows_done;          /* nonzero: z_fwd / z_kl / scal were already produced by the caller (lbbnn_layers_dense_flows,
                                lbbnn_flow_chain): lbbnn_layers_operands then runs K1 only for this layer */
    /* split == 2 (LBBNN_F_F16S operands): per-output-feature accumulator scales written by K1, (O) floats each, exact
       powers of two: e_w row o holds fp16 hi + lo of e_w[o,:] / e_scale[o], var_w row o of var_w[o,:] / v_scale[o] */
    float *e_scale, *v_scale;
} lbbnn_layer_desc_t;

int lbbnn_layers_prepare(const lbbnn_layer_desc_t* layers, int n, const uint64_t* rng, void* stream);
/* The same forward with K5 moved to the END (it feeds no GEMM):  lbbnn_layers_operands = K3 + K1 of all layers;
 * lbbnn_layers_finalize = K5 of every layer with want_kl, kl_total = sum of the layer KLs in layer order (NULL = no
 * total; needs want_kl on every layer otherwise) and rng offset += advance, all in ONE single-workgroup launch.
 * A network forward is then 6 launches: operands (2), three GEMMs, finalize. */
int lbbnn_layers_operands(const lbbnn_layer_desc_t* layers, int n, const uint64_t* rng, void* stream);
int lbbnn_layers_finalize(const lbbnn_layer_desc_t* layers, int n, uint64_t* rng, uint64_t advance, float* kl_total,
                          void* stream);

/* The same forward with two launches fewer (what BayesianNetwork.forward uses):
 *
 * lbbnn_layers_operands_snap = lbbnn_layers_operands, and the weight-pass launch also copies the live Philox state
 *   {seed, offset} to rng_snap (2 words) and adds `advance` to the live offset.  It follows the last kernel of the
 *   forward that reads the live state (the flow kernels), so every LATER kernel of this forward -- the GEMMs, the KL
 *   finalize -- must be given rng_snap as its `rng`.  rng == NULL: no RNG in use, nothing is copied.
 *
 * The first GEMM of the forward (lbbnn_lrt_gemm_ex, lbbnn_gemm_desc_t::layers .. advance below) then carries the work of
 *   lbbnn_layers_finalize in its own launch, RNG advance included.  That is what lets lbbnn_layers_operands_snap run with
 *   advance = 0 -- and only then do its workgroups compute the planar flows of the layers THEMSELVES from the live
 *   {seed, offset} (no K3 launch ahead of the weight pass; weight_pass.hip): the advance has to come from a later launch of
 *   the same forward, none of whose kernels reads the live offset (they are given rng_snap).
 */
int lbbnn_layers_operands_snap(const lbbnn_layer_desc_t* layers, int n, uint64_t* rng, uint64_t* rng_snap,
                               uint64_t advance, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Ensemble evaluation (test_ensemble, LBBNN-GP-MF-MNF.py:286-294 / ...LRT.py:241-247: TEST_SAMPLES stochastic forwards of
 * the same batch): `members` forwards of a layer in ONE launch per kernel kind, member m bit-identical to the m-th of
 * `members` consecutive single forwards (whose shared Philox offset advances by member_advance each).
 *
 * lbbnn_ensemble_operands: K3 + K1 for all n layers and all members (2 launches): per layer, z_fwd points to
 *   [members][lbbnn_operand_ld(I)] floats (member m's z_k; MNF layers with planar flows of <= 4 transforms; ignored for
 *   LRT layers) and e_w to [members][O][ld] operands (member m's e_w = mu alpha z_m); var_w, bias_var are shared (one copy).
 *   Every layer must have stochastic = 1, want_kl = 0 (evaluation draws no KL, ...MNF.py:208), flows_done = 0, no explicit
 *   eps_z.  Member m draws from Philox offset rng[1] + m * member_advance.
 * lbbnn_lrt_gemm_members: the dual-moment GEMM of lbbnn_lrt_gemm for every member, gridDim.z = members:
 *   x + m * x_mstride (floats; 0 = the same input for every member, the first layer), e_w + m * w_mstride (floats),
 *   var_w shared, out + m * o_mstride; in-kernel noise only, at offset rng[1] + m * member_advance.
 * The caller advances rng by members * member_advance afterwards (lbbnn_rng_advance). */
int lbbnn_ensemble_operands(const lbbnn_layer_desc_t* layers, int n, int members, const uint64_t* rng,
                            uint64_t member_advance, void* stream);
int lbbnn_lrt_gemm_members(const float* x, int ldx, int64_t x_mstride, const void* e_w, int64_t w_mstride,
                           const void* var_w, int ld, const float* bias_mean, const float* bias_var,
                           const uint64_t* rng, uint32_t rng_stream, int64_t row_offset, uint64_t member_advance,
                           float* out, int ldo, int64_t o_mstride, int B, int I, int O, int flags, int members,
                           void* stream);

/* Network KL (BayesianNetwork.kl(), …LRT.py:213-214) of a network deeper than one batched launch holds.  A network of n layers issues its batched calls in
 * ceil(n / LBBNN_MAX_LAYERS) groups of consecutive layers; each group's KL finalize writes its layers' values into ONE
 * contiguous buffer kl_layers[0..n), and this call forms *total = ((0 + kl_layers[0]) + kl_layers[1]) + ... in fp32 -- the
 * order and precision in which the finalize of a single group adds its total.  1 <= n <= LBBNN_MAX_DEPTH; one launch of one
 * thread, no host read: capturable.  total may be kl_layers + n. */
#define LBBNN_MAX_DEPTH 16
int lbbnn_kl_total(const float* kl_layers, int n, float* total, void* stream);

/* Left folds of short rows: out[r] = ((0 + v[r * ld + 0]) + v[r * ld + 1]) + ... + v[r * ld + n - 1] in fp32 for r < rows.
 * The log-probability totals of a baseline network of more than three layers: its layers' lbbnn_gate_sample_draw calls write
 * log_prior into v[0][i] and log_q into v[1][i] of one [2][n] buffer, and one call (rows = 2) forms both network totals in
 * layer order -- what the chain of fp32 adds of a three-layer network forms.  One launch, one thread per row, plain stores,
 * no atomics, no LDS, no host read: deterministic and capturable.  out must not overlap v.
 * Checks, before the launch: v / out NULL: LBBNN_E_NULL; rows outside [1, LBBNN_FOLD_MAX_ROWS], n outside
 * [1, LBBNN_FOLD_MAX_N], ld < n: LBBNN_E_SHAPE; a pointer off 4 bytes: LBBNN_E_ALIGN. */
#define LBBNN_FOLD_MAX_ROWS 64       /* one wave: the caller folds 2 rows */
#define LBBNN_FOLD_MAX_N 64          /* a serial fold per thread: meant for one value per layer (n <= LBBNN_MAX_DEPTH) */
int lbbnn_fold_rows(const float* v, int rows, int n, int ld, float* out, void* stream);


/* ---------------------------------------------------------------------------------------------
 * K6  lbbnn_gate_sample -- baseline LBBNN layer (explicit latent-binary gate x Gaussian weight sample).
 *
 * Replaces, for BayesianLinear.forward of LBBNN-GP-MF.py:228-255, ONE fused pass over (O,I):
 *   ws = mu + softplus(rho)*eps ; weight = cgamma*ws        Gaussian.rsample :85-87, :232-233   (mode 0)
 *   weight = cgamma*mu (mode 1, medimean :236-238) | alpha_attr*mu (mode 2, :240-242)
 *   bias = bias_mu + softplus(bias_rho)*eps_b  (mode 0) | bias_mu
 * and, when want_lp, the Monte-Carlo log-probabilities (:246-251):
 *   log_prior = GaussGamma(weight_a,weight_b).log_prob(weight,cgamma)        :140-151
 *             + GaussGamma(bias_a,bias_b).log_prob(bias,1) + BetaBinomial(pa,pb).log_prob(cgamma)  :162-173
 *   log_q     = Gaussian.full_log_prob(weight,cgamma) :99-101 + Bernoulli(gamma_alpha).log_prob(cgamma) :122-128
 *             + Gaussian.log_prob(bias) :89-92
 * The Gamma draws tau_w (1) / tau_b (O) of :141 are inputs (drawn by the host wrapper with torch).
 * exact bits (the reference's `.exact` switches, :559-627): 1 weight_prior, 2 bias_prior, 4 gamma_prior, 8 gamma.
 * Outputs: w_out = GEMM operand [O][ld] (fp32, or the split bf16 hi|lo layout with LBBNN_F_SPLIT16) for
 *          lbbnn_lrt_gemm(LBBNN_F_MEAN_ONLY) = F.linear (:255); bias_out (O); log_prior, log_q (1 float each);
 *          rows: workspace of 4*O floats.  eps_w (O,I) / eps_b (O) NULL => Philox (streams EPS_W / EPS_B).
 */
#define LBBNN_STREAM_EPS_W 4
#define LBBNN_STREAM_EPS_B 5
#define LBBNN_MODE_SAMPLE 0
#define LBBNN_MODE_MEDIMEAN 1
#define LBBNN_MODE_MEAN 2

typedef struct lbbnn_gate_args {
    const float *mu, *rho, *gamma_alpha, *cgamma, *eps_w, *alpha_attr;       /* (O,I) */
    const float *bias_mu, *bias_rho, *eps_b, *bias_a, *bias_b, *tau_b;       /* (O)   */
    const float *weight_a, *weight_b, *tau_w, *pa, *pb;                      /* (1)   */
    void* w_out; float* bias_out; float* rows; float* log_prior; float* log_q;
    int O, I, ld, mode, exact, want_lp, flags;
    uint32_t layer_id;
} lbbnn_gate_args_t;

int lbbnn_gate_sample(const lbbnn_gate_args_t* args, const uint64_t* rng, void* stream);

/* K6b  lbbnn_gate_backward -- backward of the SAMPLED baseline layer (mode LBBNN_MODE_SAMPLE with log-probabilities: what
 * net.sample_elbo(...)[0].backward() differentiates, LBBNN-GP-MF.py:331-337).  Inputs: the forward's arguments (eps_w /
 * eps_b explicit, or NULL + the forward's rng state: same Philox streams), dW (O,I) = G^T x of F.linear (NULL = 0),
 * g_sum (O) = column sums of G (NULL = 0), and the device scalars g_lp = dL/dlog_prior, g_lq = dL/dlog_q (NULL = 0).
 * Outputs: d_mu, d_rho, d_cgamma, d_alpha (O,I) [d_alpha: through Bernoulli.log_prob's alpha, :125-127]; d_bias_mu,
 * d_bias_rho, d_bias_a, d_bias_b, d_tau_b (O); d_scalars[5] = d weight_a, d weight_b, d tau_w, d pa, d pb; w_out (O,I,
 * nullable): the sampled weight as a dense fp32 matrix (the operand of dX = G W).  rows: 3*O floats of workspace.
 * `exact` bits as in the forward (a rounded, detached gate passes no gradient).  Two launches. */
typedef struct lbbnn_gate_bwd_args {
    const float *mu, *rho, *gamma_alpha, *cgamma, *eps_w;                    /* (O,I) */
    const float *bias_mu, *bias_rho, *eps_b, *bias_a, *bias_b, *tau_b;       /* (O)   */
    const float *weight_a, *weight_b, *tau_w, *pa, *pb;                      /* (1)   */
    const float *dW, *g_sum, *g_lp, *g_lq;
    float *d_mu, *d_rho, *d_cgamma, *d_alpha, *w_out;
    float *d_bias_mu, *d_bias_rho, *d_bias_a, *d_bias_b, *d_tau_b, *d_scalars, *rows;
    int O, I, exact;
    uint32_t layer_id;
} lbbnn_gate_bwd_args_t;

int lbbnn_gate_backward(const lbbnn_gate_bwd_args_t* args, const uint64_t* rng, void* stream);

/* K6 / K6b with in-kernel draws -- the baseline layer's whole stochastic input from the Philox state `rng` (required):
 *   alpha = sigmoid(lambdal); u = uniform(stream GATE, counter (o, i/4))[i%4];
 *   c = clipped_sigmoid((logit(clamp_probs(alpha)) + log u' - log1p(-u')) / temperature), u' = clamp_probs(u)
 *       (torch's RelaxedBernoulli.rsample, LBBNN-GP-MF.py:300-302); exact bit 8 (gamma.exact): c = (u < alpha), the hard draw;
 *   tau_w = Gamma(weight_a, weight_b) (stream GAMMA_W, element 0), tau_b[o] = Gamma(bias_a[o], bias_b[o]) (stream GAMMA_B,
 *       element o)  (:141; Marsaglia-Tsang on Philox normals / uniforms, counter (element, attempt), at most
 *       LBBNN_GAMMA_MAX_ATTEMPTS attempts; a NaN / non-positive / infinite shape gives NaN);
 *   eps_w / eps_b as lbbnn_gate_sample (explicit or streams EPS_W / EPS_B).
 * lbbnn_gate_sample_draw: `g` as for lbbnn_gate_sample with mode LBBNN_MODE_SAMPLE and want_lp = 1; g.gamma_alpha, g.cgamma,
 * g.alpha_attr, g.tau_w, g.tau_b are not read.  Outputs in addition to g's: gammas (O,I) = c, alpha (O,I, nullable) = alpha,
 * tau_w (1), tau_b (O).  Two launches, as lbbnn_gate_sample.
 * lbbnn_gate_backward_draw: `g` as for lbbnn_gate_backward with the forward's tau_w / tau_b outputs in g.tau_w / g.tau_b;
 * g.gamma_alpha, g.cgamma, g.d_cgamma, g.d_alpha, g.d_tau_b are not read / written (d_tau_b may be given).  Writes
 * d_lambdal = alpha (1 - alpha) (d alpha + d c * dc/dalpha) and adds the Gamma reparameterisation terms
 * (d tau * g(x, a) / b and -d tau * tau / b, x = b tau, g of lbbnn_gamma_grad) to d weight_a / d weight_b / d bias_a / d bias_b.
 * Two launches, as lbbnn_gate_backward. */
#define LBBNN_STREAM_GATE 8
#define LBBNN_STREAM_GAMMA_W 9
#define LBBNN_STREAM_GAMMA_B 10
#define LBBNN_GAMMA_MAX_ATTEMPTS 32

typedef struct lbbnn_gate_draw_args {
    lbbnn_gate_args_t g;
    const float* lambdal;                     /* (O,I) */
    float *gammas, *alpha;                    /* (O,I) out; alpha nullable */
    float *tau_w, *tau_b;                     /* (1), (O) out */
    float temperature;
} lbbnn_gate_draw_args_t;

int lbbnn_gate_sample_draw(const lbbnn_gate_draw_args_t* args, const uint64_t* rng, void* stream);

typedef struct lbbnn_gate_bwd_draw_args {
    lbbnn_gate_bwd_args_t g;
    const float* lambdal;                     /* (O,I) */
    float* d_lambdal;                         /* (O,I) out */
    float temperature;
} lbbnn_gate_bwd_draw_args_t;

int lbbnn_gate_backward_draw(const lbbnn_gate_bwd_draw_args_t* args, const uint64_t* rng, void* stream);

/* Reproduce the in-kernel draws of the two kernels above (tests):
 * lbbnn_philox_uniform: out[r][c] = uniform(counter (row_base + r, c/4))[c%4], the gate's indexing; uniform(bits) =
 *   ((bits >> 8) + 0.5) * 2^-24, in (0, 1).  rows > 0.
 * lbbnn_philox_std_gamma: out[i] = standard Gamma(a[i]) draw of element i (counter (i, attempt)) divided by rate[i]
 *   (rate NULL = 1) and clamped below at FLT_MIN as torch's Gamma.rsample does.
 * lbbnn_gamma_grad: out[i] = g(x[i], a[i]) = -(dF(x; a)/da) / f(x; a), F / f the standard Gamma cdf / density: the
 *   implicit reparameterisation gradient dx/da that lbbnn_gate_backward_draw uses (fp64 series; relative error ~1e-16 / Q(a, x)). */
int lbbnn_philox_uniform(const uint64_t* rng, uint32_t rng_stream, int64_t row_base, int64_t rows, int64_t cols, float* out,
                         void* stream);
int lbbnn_philox_std_gamma(const uint64_t* rng, uint32_t rng_stream, const float* a, const float* rate, int64_t n, float* out,
                           void* stream);
int lbbnn_gamma_grad(const float* x, const float* a, int64_t n, float* out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Ensemble evaluation of the baseline LBBNN (test_ensemble / outofsample, LBBNN-GP-MF.py:345-502): `members` stochastic
 * forwards of one batch in 1 + n launches instead of 2 + 1 per layer and member.
 *
 * lbbnn_gate_members: the gate x Gaussian weight draw of every layer and every member in ONE launch (one workgroup per
 *   output row of each layer; mu, rho, lambdal read once, alpha = sigmoid(lambdal) and sigma = softplus(rho) computed once).
 *   Member m draws from the Philox state {rng[0], rng[1] + m * member_advance} with the streams and counters of
 *   lbbnn_gate_sample_draw: gate uniform from stream GATE*64 + layer_id at counter (o, i/4), eps_w from EPS_W*64 + layer_id,
 *   eps_b from EPS_B*64 + layer_id.  Gates:
 *     gates = LBBNN_GATES_SAMPLE: c as lbbnn_gate_sample_draw draws it (the hard draw u < alpha when exact bit 8 is set,
 *             else the relaxed gate at `temperature`, which must then be > 0);
 *     gates = LBBNN_GATES_MPM:    c = (alpha > 0.5), the median probability model (outofsample(medimod=True), :469-473).
 *   w = c * (mu + sigma * eps_w) and bias = bias_mu + softplus(bias_rho) * eps_b: member m's w_out and bias_out are bitwise
 *   what lbbnn_gate_sample_draw writes at offset rng[1] + m * member_advance.  No log-probabilities, no Gamma draws.
 *   Per layer: w_out [members][O][ld] GEMM operands (fp32, or the split bf16 hi|lo layout with LBBNN_F_SPLIT16; zero tail
 *   [I, ld); 16-B aligned), bias_out [members][O]; nullable gate_rows [members][O] = sum_i c (fixed summation order: bitwise
 *   reproducible) and gates [members][O][I] = c.  ld a multiple of 32, I <= ld <= 4096.  rng is required (LBBNN_E_NOISE).
 * lbbnn_gemm_members_mean: the mean-only product out = x . w^T + bias of lbbnn_lrt_gemm(LBBNN_F_MEAN_ONLY) for every member,
 *   gridDim.z = members: x + m * x_mstride (0 = the same input for every member), w + m * w_mstride, bias + m * b_mstride
 *   (floats; bias nullable), out + m * o_mstride.  Member m is bitwise the single lbbnn_lrt_gemm call on its slices.
 *   flags: LBBNN_F_RELU | LBBNN_F_SPLIT16 | LBBNN_F_LOG_SOFTMAX (O <= 16); LBBNN_F_MEAN_ONLY is implied.  x_mstride,
 *   w_mstride and o_mstride multiples of 4 (every member 16-B aligned); o_mstride >= B * ldo.  1 <= members <= 65535. */
#define LBBNN_GATES_SAMPLE 0
#define LBBNN_GATES_MPM 1

typedef struct lbbnn_gate_member_desc {
    const float *mu, *rho, *lambdal;          /* (O,I) */
    const float *bias_mu, *bias_rho;          /* (O)   */
    void* w_out;                              /* [members][O][ld] */
    float* bias_out;                          /* [members][O]     */
    float* gate_rows;                         /* [members][O], nullable */
    float* gates;                             /* [members][O][I], nullable */
    int O, I, ld, flags, exact;               /* flags: 0 | LBBNN_F_SPLIT16; exact: the layer's exact bits (8 = gamma) */
    uint32_t layer_id;
} lbbnn_gate_member_desc_t;

int lbbnn_gate_members(const lbbnn_gate_member_desc_t* layers, int n, int members, int gates, float temperature,
                       const uint64_t* rng, uint64_t member_advance, void* stream);
int lbbnn_gemm_members_mean(const float* x, int ldx, int64_t x_mstride, const void* w, int64_t w_mstride, int ld,
                            const float* bias, int64_t b_mstride, float* out, int ldo, int64_t o_mstride,
                            int B, int I, int O, int flags, int members, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Ensemble evaluation of variational dropout (variational_dropout.py:154-160: num_test_ensemble_samples forwards of one
 * batch).  theta is shared by every member (no per-member weight draw), so one lbbnn_vd_operands per layer serves all members.
 *
 * lbbnn_vd_gemm_members: the dual-moment GEMM of lbbnn_lrt_gemm with var_scale (alpha) and no bias for `members` members:
 *   out[m][b][o] = mean + sqrt(var * var_scale[o]) * eps_m (+ReLU), e_w / var_w shared (lbbnn_vd_operands), eps_m the in-kernel
 *   draw at Philox offset rng[1] + m * member_advance (stream rng_stream, row row_offset + b, column group o/4).
 *   fanout = 0: gridDim.z = members; member m reads x + m * x_mstride and writes out + m * o_mstride.
 *   fanout = 1: x_mstride must be 0 (the same input for every member: the first layer); the grid has no member dimension --
 *     each workgroup computes its tile's two products once and writes every member's out + m * o_mstride.
 *   Either way member m is bitwise the single lbbnn_lrt_gemm(var_scale) call at offset rng[1] + m * member_advance: the kernel
 *   and tile are the ones that call picks (fp32, LDS-DMA, bf16x3 with LBBNN_F_SPLIT16 [| LBBNN_F_SINGLE16 [| LBBNN_F_HALF16]],
 *   or the O <= 16 kernel).  flags: LBBNN_F_RELU | LBBNN_F_SPLIT16 | LBBNN_F_SINGLE16 | LBBNN_F_HALF16, else LBBNN_E_FLAGS.
 *   1 <= members <= 65535 and fanout in {0, 1} (LBBNN_E_SHAPE); strides >= 0, o_mstride >= B * ldo (LBBNN_E_SHAPE), x_mstride
 *   and o_mstride multiples of 4 (LBBNN_E_ALIGN); rng required (LBBNN_E_NOISE).  The caller advances rng afterwards. */
int lbbnn_vd_gemm_members(const float* x, int ldx, int64_t x_mstride, const void* e_w, const void* var_w, int ld,
                          const float* var_scale, const uint64_t* rng, uint32_t rng_stream, int64_t row_offset,
                          uint64_t member_advance, float* out, int ldo, int64_t o_mstride,
                          int B, int I, int O, int flags, int members, int fanout, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Frozen evaluation model of an LRT / MNF network: the GEMM operands taken ONCE from the trained parameters, with the gates
 * as trained or thresholded (the median probability model of outofsample(net, loader, medimod=True),
 * LBBNN-GP-MF-LRT.py:295-314, LBBNN-GP-MF-MNF.py:342-366), which the member GEMMs above then evaluate without reading the
 * parameters again.
 *
 * Per weight, with sigma = log1p(exp(weight_rho)), alpha = 1/(1+exp(-lambdal)) and the gate value a:
 *   mode = LBBNN_FROZEN_ALPHA: a = alpha -- the evaluation forward (...LRT.py:167-180, ...MNF.py:191-206); the operands are
 *                              the values lbbnn_weight_pass writes (the same device functions in the same order);
 *   mode = LBBNN_FROZEN_MPM:   a = 1 where lambdal > cut, else 0, compared in fp32; cut = logit(threshold), 0 for the
 *                              median model alpha > 0.5.  (An fp32 sigmoid(lambdal) > 0.5 differs only for 0 < lambdal <
 *                              ~6e-8, where the rounded alpha is exactly 0.5; NaN is never kept.)
 *   E0 = weight_mu * a (mpm: weight_mu itself or +0.0),  V = sigma^2 * a^2 (mpm: sigma^2 or 0).  The bias is never gated.
 *
 * lbbnn_frozen_operands: ONE launch for all n <= LBBNN_MAX_LAYERS layers.  Per layer it reads weight_mu, weight_rho, lambdal
 *   (O,I) and bias_rho (O) once and writes
 *     e0        [O][ld] plain fp32 E0, zero tail [I, ld);
 *     e_w       [O][ld] GEMM operand of E0 (fp32, or the bf16 hi | lo layout with LBBNN_F_SPLIT16 in flags): what an LRT
 *               layer, and an MNF layer at z = 1, multiply with;
 *     var_w     [O][ld] GEMM operand of V in the same format;   bias_var (O) = softplus(bias_rho)^2;
 *     kept_rows (O) int32: the number of weights of the row with lambdal > cut, in BOTH modes.
 *   All five outputs are required (LBBNN_E_NULL).  1 <= I <= ld (LBBNN_E_SHAPE), ld a multiple of 32, e0 / e_w / var_w 16-B
 *   aligned, every other pointer 4-B aligned (LBBNN_E_ALIGN); LBBNN_F_SPLIT16 needs I % 4 == 0 and 16-B aligned parameters
 *   (LBBNN_E_ALIGN), fp32 operands take any I.  flags other than 0 | LBBNN_F_SPLIT16, or an unknown mode: LBBNN_E_FLAGS.
 *   The fields q0_mean ... e_w_members are not read by this call.
 *
 * lbbnn_frozen_members: the per-member part, for the MNF layers among the n descriptors (q0_mean != NULL; LRT layers are
 *   skipped -- their e_w is shared by every member: lbbnn_lrt_gemm_members takes w_mstride = 0).  Member m's z_k is drawn and
 *   pushed through the planar z_flow exactly as lbbnn_ensemble_operands does it (Philox offset rng[1] + m * member_advance,
 *   stream LBBNN_STREAM_EPS_Z * 64 + layer_id; more than one member needs z_flow.T <= 4) into z_fwd + m * z_mstride, then ONE
 *   launch writes e_w_members + m * O * ld = operand(E0 * z_m) (format by flags) for every member and MNF layer.  z is not
 *   gated.  When all MNF layers have the same z_mstride (their z blocks side by side in one [members][z_mstride] buffer) the
 *   flows of all layers are one launch, else one launch per layer.
 *   1 <= members <= 65535, 1 <= I <= ld, I <= z_mstride, 0 <= z_flow.T <= LBBNN_MAX_FLOW_T (LBBNN_E_SHAPE); I, z_mstride
 *   multiples of 4, ld of 32, e0 / z_fwd / e_w_members 16-B aligned (LBBNN_E_ALIGN); rng == NULL with an MNF layer present:
 *   LBBNN_E_NOISE.  No MNF layer: a successful no-op.  The caller advances rng afterwards, as for lbbnn_ensemble_operands. */
#define LBBNN_FROZEN_ALPHA 0
#define LBBNN_FROZEN_MPM 1

typedef struct lbbnn_frozen_desc {
    const float *weight_mu, *weight_rho, *lambdal;   /* (O,I) */
    const float *bias_rho;                           /* (O)   */
    const float *q0_mean, *q0_log_var;               /* (I); both NULL for an LRT layer */
    lbbnn_planar_flow_t z_flow;                      /* MNF layers: the planar z flow   */
    float* e0;                                       /* [O][ld] fp32                    */
    void *e_w, *var_w;                               /* [O][ld] GEMM operands           */
    float* bias_var;                                 /* (O)                             */
    int32_t* kept_rows;                              /* (O)                             */
    float* z_fwd;                                    /* MNF: member m's z at z_fwd + m * z_mstride (I floats used) */
    void* e_w_members;                               /* MNF: [members][O][ld] GEMM operands */
    int64_t z_mstride;                               /* floats                          */
    int O, I, ld;
    int flags;                                       /* 0 | LBBNN_F_SPLIT16             */
    int mode;                                        /* LBBNN_FROZEN_ALPHA | LBBNN_FROZEN_MPM */
    float cut;                                       /* logit(threshold), LBBNN_FROZEN_MPM and kept_rows */
    uint32_t layer_id;
} lbbnn_frozen_desc_t;

int lbbnn_frozen_operands(const lbbnn_frozen_desc_t* layers, int n, void* stream);
int lbbnn_frozen_members(const lbbnn_frozen_desc_t* layers, int n, int members, const uint64_t* rng,
                         uint64_t member_advance, void* stream);

/* ---------------------------------------------------------------------------------------------
 * K4m  lbbnn_flow_dense_members -- z of every member of an evaluation ensemble through the DENSE coupling z flows (RNVP /
 * MNF type, flows2.py:188-241; the reference's default Z_FLOW_TYPE, LBBNN-GP-MF-MNF.py:46) of up to LBBNN_MAX_LAYERS MNF
 * layers in ONE launch, whatever the member count: grid = (ceil(members / 16), n), one workgroup carries 16 members of one
 * layer through the whole chain with z resident in LDS, the affine steps on v_mfma_f32_16x16x4_f32 (exact fp32) with the
 * members as the 16 columns, so every coupling matrix is read once per 16 members.
 *
 * Draw contract: member m is the forward-draw z of the single forward (lbbnn_layers_dense_flows with draw_masks = 1, no
 * explicit eps) at Philox state {seed, off} = {rng[0], rng[1] + m * member_advance}, with lid = layer_id & 63:
 *   eps_i = philox_normal4(seed, off, LBBNN_STREAM_EPS_Z * 64 + lid, counter (i / 4, 0))[i % 4]
 *   z0_i  = q0_mean_i + sqrtf(expf(q0_log_var_i)) * eps_i                       (LBBNN-GP-MF-MNF.py:183-185)
 *   mask of transform t at element i = bit t of word 0 of philox_bits4(seed, off, LBBNN_STREAM_MASK * 64 + lid, counter (i, 0))
 *   (words 1 / 2 are the KL branch's and the r flow's masks: evaluation draws neither), then the T transforms of
 *   flows2.py:206-219 (RNVP) / :233-241 (MNF type).  Same draws as the single forward; the sums of the affine steps run on
 *   the matrix cores in another order than its GEMVs, so z is equal to fp32 rounding, not bit for bit.  A member's z does
 *   not depend on `members` or on its position (chunks of an ensemble give the same bits as one call).
 * Only z is written (z_fwd + m * z_mstride, I floats); no log-determinant (evaluation draws no KL, ...MNF.py:208).
 * mask_out: NULL, or [members][T][I] floats in {0,1}: the masks used.  zt: T transforms of ONE kind; their mask_fwd /
 * mask_kl fields are ignored.
 * Checks, before any launch: NULL layers / q0_mean / q0_log_var / z_fwd / zt / a transform's matrices: LBBNN_E_NULL;
 * rng == NULL: LBBNN_E_NOISE; 1 <= n <= LBBNN_MAX_LAYERS, 1 <= members <= 65535, 0 <= T <= LBBNN_MAX_DENSE_T,
 * 1 <= I <= lbbnn_flow_dense_members_max_dim() (LDS: 1.25 KiB per 16 elements of z -- the z image and one byte of mask bits
 * per element and member -- plus 49 KiB for the hidden matrices and partials, within 160 KiB), 1 <= hidden <=
 * LBBNN_MAX_HIDDEN, z_mstride >= I, a kind other than LBBNN_FLOW_RNVP / LBBNN_FLOW_MNF or kinds mixed within a layer:
 * LBBNN_E_SHAPE; I % 4, z_mstride % 4, z_fwd off a 16-B boundary: LBBNN_E_ALIGN.
 *
 * lbbnn_frozen_members_dense: lbbnn_frozen_members for a frozen model whose MNF layers have dense z flows: F[i] describes
 *   the z flow of layers[i] (entries of LRT layers, q0_mean == NULL in layers[i], are not read); z_fwd and z_mstride are
 *   taken from layers[i], whose z_flow field is ignored.  One lbbnn_flow_dense_members launch for all MNF layers, then the
 *   launch of lbbnn_frozen_members that writes e_w_members + m * O * ld = operand(E0 * z_m).  The checks of both. */
typedef struct lbbnn_dense_members {
    const float *q0_mean, *q0_log_var;               /* (I)                                                    */
    const lbbnn_dense_transform_t* zt;               /* T transforms (host array); mask_fwd / mask_kl ignored  */
    int T, I;
    uint32_t layer_id;
    float* z_fwd;                                    /* member m's z at z_fwd + m * z_mstride                  */
    int64_t z_mstride;                               /* floats                                                 */
    float* mask_out;                                 /* NULL, or [members][T][I]                               */
} lbbnn_dense_members_t;

int lbbnn_flow_dense_members_max_dim(void);
int lbbnn_flow_dense_members(const lbbnn_dense_members_t* layers, int n, int members, const uint64_t* rng,
                             uint64_t member_advance, void* stream);
int lbbnn_frozen_members_dense(const lbbnn_frozen_desc_t* layers, const lbbnn_dense_members_t* flows, int n, int members,
                               const uint64_t* rng, uint64_t member_advance, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Compact median-probability model: the frozen model of the units some output depends on.  A hidden unit or input feature
 * whose every consumer weight is pruned (or whose consumers are themselves unneeded) leaves with its whole row and column;
 * what remains computes the same function with smaller dense GEMMs (lbbnn_lrt_gemm_members / lbbnn_lrt_gemm at the compact
 * shapes).  A compact layer is described by the full layer's parameters plus a map: the sorted row and column indices that
 * stay.  The caller builds the maps (evaluate.live_structure); the kernels read them as given.
 *
 * lbbnn_frozen_operands_compact: lbbnn_frozen_operands for compact layers, ONE launch for all n <= LBBNN_MAX_LAYERS layers.
 *   layers[i].O / I / ld are the COMPACT sizes O' / I' / ld'; the parameter pointers address the full (O_full, I_full)
 *   arrays; mode must be LBBNN_FROZEN_MPM (LBBNN_E_FLAGS otherwise: alpha gates are never exactly zero).  Compact element
 *   (o', j') is the element of lbbnn_frozen_operands at (rows[o'], cols[j']):
 *     e0, e_w, var_w [O'][ld'] with a zero tail [I', ld');  bias_var[o'] = softplus(bias_rho[rows[o']])^2;
 *     kept_rows[o'] = the number of j' < I' with lambdal[rows[o']][cols[j']] > cut.
 *   Checks, before any launch: those of lbbnn_frozen_operands; maps / rows / cols NULL: LBBNN_E_NULL; O' > O_full or
 *   I' > I_full: LBBNN_E_SHAPE; LBBNN_F_SPLIT16 needs I' % 8 == 0 (LBBNN_E_ALIGN; fp32 operands take any I').
 *
 * lbbnn_frozen_members_compact: lbbnn_frozen_members for a compact model.  The descriptors carry the FULL-width q0_mean,
 *   q0_log_var, planar z_flow and z_fwd / z_mstride (>= I_full); the flow launch is the one of lbbnn_frozen_members at width
 *   maps[i].I_full, then ONE launch writes e_w_members + m * O' * ld' = operand(e0'[o'][j'] * z_m[cols[j']]) for every
 *   member and MNF layer: the gather of z is fused into that launch, no compact z is stored.  The checks of
 *   lbbnn_frozen_members (I' % 4, and I_full % 4 for the flow) plus the map checks above.
 *
 * Draw contract of a compact model:
 *   - z: drawn at the full width from the same Philox stream, offsets and counters as lbbnn_frozen_members, so member m's z
 *     is bit for bit the full model's;
 *   - eps_out of compact layer i: stream LBBNN_STREAM_EPS_OUT * 64 + layer_id, counter (row_offset + b, j' / 4) with j' the
 *     COMPACT column (the GEMMs index the noise by the column they compute).  A stochastic member of a compact model
 *     therefore equals the full median-probability member in distribution, not in numbers;
 *   - the posterior-mean forward draws no eps_out: it equals the full model's to fp32 rounding (the order of the sums).
 *
 * lbbnn_gather_columns: out[b][j] = x[b][idx[j]] for b < B, j < n_idx; columns [n_idx, ldo) of out are written as zeros.
 *   B == 0 is a successful no-op.  NULL x / idx / out: LBBNN_E_NULL; n_idx < 1, ldo < n_idx, ldx < 1, B < 0:
 *   LBBNN_E_SHAPE; out off a 16-B boundary, ldo % 4 != 0: LBBNN_E_ALIGN.  idx holds column indices of x in [0, ldx). */
typedef struct lbbnn_compact_map {
    const int32_t* rows;                             /* (O') indices into [0, O_full) */
    const int32_t* cols;                             /* (I') indices into [0, I_full) */
    int O_full, I_full;
} lbbnn_compact_map_t;

int lbbnn_frozen_operands_compact(const lbbnn_frozen_desc_t* layers, const lbbnn_compact_map_t* maps, int n, void* stream);
int lbbnn_frozen_members_compact(const lbbnn_frozen_desc_t* layers, const lbbnn_compact_map_t* maps, int n, int members,
                                 const uint64_t* rng, uint64_t member_advance, void* stream);
int lbbnn_gather_columns(const float* x, int ldx, const int32_t* idx, int n_idx, float* out, int ldo, int B, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Sparse median-probability model: the kept weights of LBBNN_FROZEN_MPM alone, in CSR, evaluated by a vector-ALU kernel that
 * touches no pruned weight.  Per layer, with the keep rule of lbbnn_frozen_operands (lambdal > cut compared in fp32, NaN is
 * never kept) and columns ascending within a row:
 *     row_ptr (O + 1) int32, the exclusive scan of kept_rows;   col (nnz) int32;
 *     mean (nnz) fp32 = weight_mu;   var (nnz) fp32 = sigma^2, sigma = log1p(exp(weight_rho)) through the device functions of
 *     lbbnn_frozen_operands, so var is bit for bit its fp32 var_w at the kept places;   bias_var (O) = softplus(bias_rho)^2.
 *
 * lbbnn_sparse_count: ONE launch for all n <= LBBNN_MAX_LAYERS layers, one wave per weight row: kept_rows[o] = the number
 *   of weights of row o with lambdal > cut.  Reads lambdal only; the caller scans kept_rows into row_ptr.
 *   NULL layers / lambdal / kept_rows: LBBNN_E_NULL; n outside [1, LBBNN_MAX_LAYERS], O <= 0, I <= 0: LBBNN_E_SHAPE; a
 *   pointer off a 4-B boundary: LBBNN_E_ALIGN.
 * lbbnn_sparse_pack: ONE launch for all n layers, one wave per weight row: 64 columns at a time the kept ones are compacted
 *   in ascending order (a ballot of the lanes and the count of the lower kept lanes give each its place) and col / mean /
 *   var are written from row_ptr[o] on, bias_var[o] once per row.  Plain vector stores, no atomics.  Nothing is written at
 *   or past `nnz` (the capacity of col / mean / var) or past row_ptr[o + 1], whatever row_ptr holds.
 *   NULL layers / weight_mu / weight_rho / lambdal / bias_rho / row_ptr / bias_var, or col / mean / var with nnz > 0:
 *   LBBNN_E_NULL; the shapes above or nnz < 0: LBBNN_E_SHAPE; a pointer off a 4-B boundary: LBBNN_E_ALIGN.
 *
 * lbbnn_frozen_members_z: the flow launch of lbbnn_frozen_members alone -- member m's z of every MNF layer among the n
 *   descriptors (q0_mean != NULL) into z_fwd + m * z_mstride, same Philox stream, offsets and counters, so z is bit for bit
 *   the z of lbbnn_frozen_members.  e0, e_w_members, ld and flags are not read; nothing is scaled.  The checks of
 *   lbbnn_frozen_members that concern the flow: NULL layers / q0_log_var / z_fwd / a transform: LBBNN_E_NULL; rng == NULL with
 *   an MNF layer present: LBBNN_E_NOISE; n, members, O, I, z_mstride < I, z_flow.T: LBBNN_E_SHAPE; I % 4, z_mstride % 4, z_fwd
 *   off a 16-B boundary: LBBNN_E_ALIGN.  No MNF layer: a successful no-op.
 *
 * lbbnn_sparse_layer_members: one layer of the sparse model for every member in ONE launch.  Activations between layers are
 *   TRANSPOSED, [member][unit][ld] with ld >= B floats, so that the 64 lanes of a wave are 64 batch rows and every load of
 *   a[col][.] and every store of a finished unit is one contiguous line; the first layer reads x^T as lbbnn_transpose_operand
 *   writes it, with a_mstride = 0.  Per (member m, row b, unit o), k running over row_ptr[o] .. row_ptr[o + 1] - 1 in order:
 *     mean = bias_mu[o] + sum_k (mean[k] * z_m[col[k]]) * a_m[col[k]][b]       (z == NULL: no z factor -- an LRT layer)
 *     var  = bias_var[o] + sum_k var[k] * a_m[col[k]][b]^2
 *     out  = mean + v_sqrt_f32(var) * eps,   or out = mean with LBBNN_F_MEAN_ONLY;   then ReLU (LBBNN_F_RELU) or, with
 *     LBBNN_F_LOG_SOFTMAX (O <= 16, row-major output), log_softmax over the row.
 *   Both sums are sequential fp32 FMAs from 0 in CSR order, the bias added last, so an output's bits depend on its member,
 *   row and unit alone -- not on B, members, chunking or the grid.  An empty row gives relu(bias_mu + sqrt(bias_var) * eps).
 *   eps = philox_normal4 at {rng[0], rng[1] + m * member_advance}, stream rng_stream, counter (row_offset + b, o / 4), word
 *   o % 4: the draw of lbbnn_lrt_gemm_members at the same (row, unit).
 *   out_rows == 0: out[m * o_mstride + o * ldo + b] (transposed, ldo >= B: the next layer's input);
 *   out_rows != 0: out[m * o_mstride + b * ldo + o] (row-major, ldo >= O: what the heads and the metrics read).
 *   B == 0: a successful no-op.  NULL row_ptr / bias_mu / bias_var / a / out, or col / mean / var with nnz > 0: LBBNN_E_NULL;
 *   B < 0, more than 65535 * 64 rows, a member's input block of 2 GiB or more, I <= 0, O <= 0, nnz < 0, members outside [1, 65535], lda < B, ldo below what the layout
 *   needs, a negative stride, z_mstride < I with more than one member: LBBNN_E_SHAPE; flags other than LBBNN_F_RELU |
 *   LBBNN_F_MEAN_ONLY | LBBNN_F_LOG_SOFTMAX, or LBBNN_F_LOG_SOFTMAX with O > 16, with LBBNN_F_RELU or with out_rows == 0:
 *   LBBNN_E_FLAGS; rng == NULL without LBBNN_F_MEAN_ONLY: LBBNN_E_NOISE; a pointer off a 4-B boundary (rng: 8 B):
 *   LBBNN_E_ALIGN.  Column indices outside [0, I) and row pointers outside [0, nnz] are clamped, never followed. */
typedef struct lbbnn_sparse_desc {
    const float *weight_mu, *weight_rho, *lambdal;   /* (O,I)                                   */
    const float *bias_rho;                           /* (O)                                     */
    const int32_t* row_ptr;                          /* (O + 1); lbbnn_sparse_pack              */
    int32_t* col;                                    /* (nnz);   lbbnn_sparse_pack              */
    float *mean, *var;                               /* (nnz);   lbbnn_sparse_pack              */
    float* bias_var;                                 /* (O);     lbbnn_sparse_pack              */
    int32_t* kept_rows;                              /* (O);     lbbnn_sparse_count             */
    int O, I;
    int nnz;                                         /* capacity of col / mean / var            */
    float cut;                                       /* logit(threshold)                        */
} lbbnn_sparse_desc_t;

int lbbnn_sparse_count(const lbbnn_sparse_desc_t* layers, int n, void* stream);
int lbbnn_sparse_pack(const lbbnn_sparse_desc_t* layers, int n, void* stream);
int lbbnn_frozen_members_z(const lbbnn_frozen_desc_t* layers, int n, int members, const uint64_t* rng,
                           uint64_t member_advance, void* stream);
int lbbnn_sparse_layer_members(const int32_t* row_ptr, const int32_t* col, const float* mean, const float* var, int nnz,
                               const float* bias_mu, const float* bias_var, const float* a, int lda, int64_t a_mstride,
                               const float* z, int64_t z_mstride, const uint64_t* rng, uint32_t rng_stream,
                               int64_t row_offset, uint64_t member_advance, float* out, int ldo, int64_t o_mstride,
                               int out_rows, int B, int I, int O, int flags, int members, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Threshold sweep of the sparse median-probability model (evaluate.threshold_sweep): the sparse models of K ascending cuts
 * c_0 < ... < c_{K-1} packed by ONE count and ONE pack launch, and evaluated by one layer launch for K x S members -- level j
 * under draw s.  Per layer with O rows the K CSRs lie level after level in one set of arrays:
 *     kept_rows (K, O) int32: kept_rows[j][o] = #{c : lambdal[o][c] > c_j}, compared in fp32 (NaN is never kept);
 *     row_ptr (K * O + 1) int32: the exclusive scan of kept_rows flattened level-major (the caller scans); level j, row o owns
 *     the slots [row_ptr[j * O + o], row_ptr[j * O + o + 1]) of the shared col / mean / var, columns ascending;
 *     mean / var / bias_var: the bits lbbnn_sparse_pack writes, so level j's segment is the model of cut c_j bit for bit.
 * The patterns are nested (a weight kept at level j is kept at every lower level) but every level has a segment of its own: a
 * member walks the kept weights of its level and nothing else.
 *
 * lbbnn_sparse_count_levels: ONE launch for all n <= LBBNN_MAX_LAYERS layers, one wave per weight row.  Each lambdal is loaded
 *   once; per 64 columns K compares against cuts in scalar registers and K ballots; kept_rows[j][o] is stored for every j.
 * lbbnn_sparse_pack_levels: ONE launch, one wave per row.  Per 64 columns lambdal is loaded once, mu / rho once for the lanes
 *   kept at level 0 (sigma computed once), and for every level the ballot and the count of the lower kept lanes give a kept
 *   lane its slot in that level's segment.  Plain vector stores, no atomics, no LDS.  Nothing is written at or past `nnz` (the
 *   capacity of col / mean / var) or past the end of a (level, row), whatever row_ptr holds.  bias_var[o] is stored once.
 *   Both: the checks and codes of lbbnn_sparse_count / lbbnn_sparse_pack; and levels outside [1, LBBNN_MAX_LEVELS], a cut that
 *   is not finite, or cuts that do not ascend strictly: LBBNN_E_SHAPE.
 *
 * lbbnn_sparse_layer_levels: lbbnn_sparse_layer_members for levels * members_per_level members in ONE launch.  Member m is
 *   level j = m / members_per_level under draw s = m % members_per_level: it reads its row pointers at row_ptr[j * O + o], its
 *   z at z + s * z_mstride, draws eps at Philox offset rng[1] + s * member_advance, reads its input at a + m * a_mstride and
 *   writes at out + m * o_mstride.  Everything else is lbbnn_sparse_layer_members (the same kernel): the sums, the counters,
 *   the heads, the clamps -- so member (j, s) has the bits of member s of the model packed for cut c_j alone, and the draws
 *   are common to the levels.  `nnz` is the capacity of col / mean / var over all levels; row_ptr holds levels * O + 1 entries.
 *   The work is proportional to the sum of the levels' kept weights.  The checks and codes of lbbnn_sparse_layer_members
 *   with members = levels * members_per_level (z_mstride < I is refused with more than one draw); and levels outside
 *   [1, LBBNN_MAX_LEVELS], members_per_level < 1 or levels * members_per_level > 65535: LBBNN_E_SHAPE. */
#define LBBNN_MAX_LEVELS 16

typedef struct lbbnn_sparse_levels_desc {
    const float *weight_mu, *weight_rho, *lambdal;   /* (O,I)                                          */
    const float *bias_rho;                           /* (O)                                            */
    const int32_t* row_ptr;                          /* (levels * O + 1); lbbnn_sparse_pack_levels     */
    int32_t* col;                                    /* (nnz);            lbbnn_sparse_pack_levels     */
    float *mean, *var;                               /* (nnz);            lbbnn_sparse_pack_levels     */
    float* bias_var;                                 /* (O);              lbbnn_sparse_pack_levels     */
    int32_t* kept_rows;                              /* (levels, O);      lbbnn_sparse_count_levels    */
    int O, I;
    int nnz;                                         /* capacity of col / mean / var, all levels       */
    int levels;                                      /* K, 1 .. LBBNN_MAX_LEVELS                       */
    float cut[LBBNN_MAX_LEVELS];                     /* logit(threshold_j), strictly ascending         */
} lbbnn_sparse_levels_desc_t;

int lbbnn_sparse_count_levels(const lbbnn_sparse_levels_desc_t* layers, int n, void* stream);
int lbbnn_sparse_pack_levels(const lbbnn_sparse_levels_desc_t* layers, int n, void* stream);
int lbbnn_sparse_layer_levels(const int32_t* row_ptr, const int32_t* col, const float* mean, const float* var, int nnz,
                              const float* bias_mu, const float* bias_var, const float* a, int lda, int64_t a_mstride,
                              const float* z, int64_t z_mstride, const uint64_t* rng, uint32_t rng_stream,
                              int64_t row_offset, uint64_t member_advance, float* out, int ldo, int64_t o_mstride,
                              int out_rows, int B, int I, int O, int flags, int levels, int members_per_level, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Frozen evaluation model of a baseline LBBNN network (LBBNN-GP-MF.py:345-502: test_ensemble and outofsample): a snapshot of
 * sigma = softplus(rho), alpha = sigmoid(lambdal) and the gated mean taken ONCE, from which every member is then drawn
 * without reading the parameters, without drawing for weights the median probability model has pruned, and -- with a map --
 * at the compact shape of the units some output depends on (evaluate.live_structure).
 *
 * lbbnn_base_frozen_operands: ONE launch for all n <= LBBNN_MAX_LAYERS layers.  layers[i].O / I / ld are the sizes O' / I' / ld'
 *   of the planes; the sources address the full (O_full, I_full) arrays (without maps: O_full = O', I_full = I').  Element
 *   (o', j') comes from (rows[o'], cols[j']) of the sources, the identity without maps.  sigma and alpha are formed by the
 *   device functions of lbbnn_gate_members (bitwise its values); keep = alpha > threshold in fp32 (NaN is never kept; at 0.5
 *   this is the c of LBBNN_GATES_MPM).  Outputs, each nullable, at least one per layer (LBBNN_E_NULL otherwise):
 *     mode = LBBNN_GATES_SAMPLE: w_mu = mu, w_sigma = sigma, e_w = operand(alpha * mu)    (the mode-2 mean, :236-238)
 *     mode = LBBNN_GATES_MPM:    w_mu = keep ? mu : +0.0, w_sigma = keep ? sigma : +0.0, e_w = operand(w_mu)  (medimean)
 *     either mode: alpha; alpha_rows[o'] = sum_j' alpha (per lane in column order, then the fixed-order wave sum: bitwise
 *     reproducible); kept_rows[o'] = sum_j' keep; b_mu = bias_mu[rows[o']]; b_sigma = softplus(bias_rho[rows[o']]);
 *     keep [O_full][I_full] uint8 in {0, 1}, rows of I_full bytes, without maps only (LBBNN_E_FLAGS with one).
 *   w_mu, w_sigma and alpha are plain fp32 [O'][ld']; e_w is fp32 or, with LBBNN_F_SPLIT16 in flags, the split bf16 hi|lo
 *   layout; every tail [I', ld') is written as zeros.  lbbnn_base_frozen_members reads alpha in SAMPLE mode only.
 *   Checks, before any launch: layers NULL, a source NULL, a map's rows / cols NULL: LBBNN_E_NULL; n outside 1 ..
 *   LBBNN_MAX_LAYERS, O' / I' < 1, ld' < I' or > 4096, O' > O_full, I' > I_full: LBBNN_E_SHAPE; ld' % 32, a plane off a 16-B
 *   boundary, any other pointer but keep off a 4-B boundary: LBBNN_E_ALIGN; an unknown mode, flags other than 0 |
 *   LBBNN_F_SPLIT16, maps with LBBNN_GATES_SAMPLE (alpha gates are never exactly zero: nothing to drop), a threshold outside
 *   (0, 1): LBBNN_E_FLAGS.
 *
 * lbbnn_base_frozen_members: every member's weights and biases of all n layers in ONE launch, from the snapshot planes.
 *   Member m draws from {rng[0], rng[1] + m * member_advance} with the streams and counters of lbbnn_gate_members, ALWAYS at
 *   the full coordinates: eps_w and the gate uniform of compact element (o', j') at counter (rows[o'], cols[j'] / 4), lane
 *   cols[j'] % 4 of streams EPS_W / GATE * 64 + layer_id; eps_b at counter (rows[o'] / 4, 0), lane rows[o'] % 4 of EPS_B * 64
 *   + layer_id.  One Philox evaluation serves every column of a lane's group that lies in the same quad of the full row.
 *     mode = LBBNN_GATES_SAMPLE: w = c * (w_mu + w_sigma * eps_w), c drawn from alpha as lbbnn_gate_members draws it (the
 *             hard draw u < alpha when exact & 8, else the relaxed gate at `temperature` > 0);
 *     mode = LBBNN_GATES_MPM:    w = w_mu + w_sigma * eps_w; a group of columns whose w_mu and w_sigma are all zero draws
 *             nothing and is stored as zeros;
 *     bias = b_mu + b_sigma * eps_b.
 *   A full model's members are bitwise those of lbbnn_gate_members from the same state (it stores -0.0 for some pruned
 *   weights where this call stores +0.0); a compact model's member weight (o', j') is bitwise the full model's at (rows[o'],
 *   cols[j']).  w_out[i]: [members][O'][ld'] fp32, or the split bf16 hi|lo layout with LBBNN_F_SPLIT16 in layers[i].flags,
 *   zero tails, 16-B aligned; bias_out[i]: [members][O']; gate_rows: NULL, or n pointers, each NULL or [members][O'] = sum_j'
 *   c (SAMPLE mode; groups of eight columns in order, each summed over the wave in a fixed order).
 *   Checks, before any launch: those of the shapes and maps above; layers / w_out / bias_out or one of their entries, b_mu,
 *   b_sigma, w_mu, w_sigma, and alpha in SAMPLE mode NULL: LBBNN_E_NULL; members outside 1 .. 65535: LBBNN_E_SHAPE; maps or
 *   gate_rows with LBBNN_GATES_SAMPLE / LBBNN_GATES_MPM respectively, temperature <= 0 in SAMPLE mode: LBBNN_E_FLAGS; rng
 *   NULL: LBBNN_E_NOISE.  The caller advances rng afterwards. */
typedef struct lbbnn_base_frozen_desc {
    const float *mu, *rho, *lambdal;          /* (O_full, I_full) sources: lbbnn_base_frozen_operands only */
    const float *bias_mu, *bias_rho;          /* (O_full) */
    float *w_mu, *w_sigma;                    /* [O'][ld'] fp32 planes */
    float* alpha;                             /* [O'][ld'] */
    void* e_w;                                /* [O'][ld'] GEMM operand of the posterior mean (format by flags) */
    float *b_mu, *b_sigma;                    /* [O'] */
    int32_t* kept_rows;                       /* [O'] */
    float* alpha_rows;                        /* [O'] */
    uint8_t* keep;                            /* [O_full][I_full], without maps only */
    int O, I, ld;                             /* O', I', ld' */
    int flags;                                /* 0 | LBBNN_F_SPLIT16: e_w, and w_out of lbbnn_base_frozen_members */
    int exact;                                /* the layer's exact bits (8 = hard gates) */
    uint32_t layer_id;
} lbbnn_base_frozen_desc_t;

int lbbnn_base_frozen_operands(const lbbnn_base_frozen_desc_t* layers, const lbbnn_compact_map_t* maps, int n, int mode,
                               float threshold, void* stream);
int lbbnn_base_frozen_members(const lbbnn_base_frozen_desc_t* layers, const lbbnn_compact_map_t* maps, int n, int members,
                              int mode, float temperature, void* w_out[], float* bias_out[], float* gate_rows[],
                              const uint64_t* rng, uint64_t member_advance, void* stream);

/* ---------------------------------------------------------------------------------------------
 * K7  lbbnn_vd_operands -- Gaussian variational-dropout layer (variational_dropout.py:55-68).
 *   phi = x.theta ; delta = (x^2).(theta^2) * alpha ; out = phi + sqrt(delta)*zeta        :64-67
 * theta is (I,O) row-major (NN layout).  This pass writes the GEMM operands theta^T and (theta^2)^T as
 * [O][ld] (fp32 or split planes) through a tiled LDS transpose, so theta^2 is never materialised in (I,O)
 * form and the same lbbnn_lrt_gemm runs with var_scale = alpha, bias = NULL.
 */
int lbbnn_vd_operands(const float* theta, void* e_w, void* var_w, int ld, int I, int O, int flags, void* stream);

/* Backward operands of a Bayesian layer from its parameters in one pass: e_t = (weight_mu * sigmoid(lambdal) * z)^T and
 * v_t = (softplus(weight_rho)^2 sigmoid(lambdal)^2)^T as GEMM operands [I][ld] with ld = lbbnn_operand_ld(O), for the
 * input-gradient products dX = G_m . W_m + 2 x (.) (G_v . W_v) (contraction over O).  z (I) NULL = LRT layer; v_t NULL =
 * posterior-mean forward.  flags: LBBNN_F_SPLIT16 as elsewhere.  Replaces lbbnn_weight_pass + 2 x lbbnn_transpose_operand. */
int lbbnn_weight_operands_t(const float* weight_mu, const float* weight_rho, const float* lambdal, const float* z,
                            void* e_t, void* v_t, int ld, int O, int I, int flags, void* stream);


/* ---------------------------------------------------------------------------------------------
 * Training support (the backward of loss.backward(), LBBNN-GP-MF-LRT.py:225).
 *
 * The training forward's GEMM is lbbnn_lrt_gemm_ex with lbbnn_gemm_desc_t::std_out: it additionally stores
 * std_out[b,o] = sqrt(var[b,o]) (pre-ReLU), which the backward needs for  dL/dvar = g * eps / (2 * std).
 *
 * lbbnn_transpose_operand: dst[c][r] = src[r][c] (squared when `square`) for src (R,C) with row stride
 * lds_src, written as a GEMM operand [C][ld] (ld = lbbnn_operand_ld(R), zero tail; fp32 or, with
 * LBBNN_F_SPLIT16, the split bf16 hi|lo layout).  With it every backward product is an "x . operand^T" GEMM on the
 * same kernels as the forward:
 *   dX  = G_m . W_m + 2 x (.) (G_v . W_v)      operands W_m^T, W_v^T          (K = O)
 *   dW_m = G_m^T . x ,  dW_v = G_v^T . x^2     operands x^T, (x^2)^T          (K = B)
 */

/* lbbnn_format_operand: dst[r][c] = src[r][c] (squared when `square`) as a GEMM operand [R][ld] (ld = lbbnn_operand_ld(C),
 * zero tail, fp32 or LBBNN_F_SPLIT16) -- no transpose: the matrix already has the contraction index contiguous.  Used by
 * the variational-dropout backward: theta (n,m) and theta^2 are the operands of dX = G . theta^T + 2 x (.) (G_v . (theta^2)^T). */
int lbbnn_format_operand(const float* src, int R, int C, int lds_src, void* dst, int ld, int square, int flags, void* stream);
int lbbnn_transpose_operand(const float* src, int R, int C, int lds_src, void* dst, int ld,
                            int square, int flags, void* stream);

/* lbbnn_weight_pass_backward (K1b): analytic backward of the fused weight pass -- one pass over (O,I).
 * Given the operand gradients from the backward GEMMs (dWm wrt e_w = mu*alpha*z_fwd, dWv wrt var_w =
 * sigma^2*alpha^2), the upstream KL gradient *g_kl (device scalar, NULL = none) and the gradients of the
 * auxiliary activations da_mu / da_var (O) (wrt act_mu / act_var, already scaled by g_kl; NULL = none), writes
 *   dmu, drho, dlambdal (O,I)              chain through alpha = sigmoid(lambda), sigma = softplus(rho)
 *   dz_fwd (I) = sum_o dWm*mu*alpha        dz_kl (I), dr0_c (I): column sums of the KL / auxiliary terms
 * Column sums are deterministic: per-row-block partials in `work` (lbbnn_weight_pass_backward_workspace floats)
 * reduced in a fixed order by a second tiny launch.  Formulas: derivative of LBBNN-GP-MF-MNF.py:195-196,211-217,230-233.
 */
typedef struct lbbnn_wpb_args {
    const float *mu, *rho, *lambdal, *dWm, *dWv;          /* (O,I); dWv may be NULL (posterior-mean forward) */
    const float *z_fwd, *z_kl, *r0_c;                     /* (I) or NULL                                     */
    const float *da_mu, *da_var;                          /* (O) or NULL                                     */
    const float *g_kl;                                    /* device scalar or NULL                           */
    lbbnn_priors_t priors;
    float *dmu, *drho, *dlambdal;                         /* (O,I) outputs                                   */
    float *dz_fwd, *dz_kl, *dr0_c;                        /* (I) outputs or NULL                             */
    float *work;
    int O, I;
    int nsplit;                                           /* dWm / dWv are nsplit slabs of (O,I), added here; 0 or 1 = plain */
    int64_t split_stride;                                 /* floats between slabs                                            */
} lbbnn_wpb_args_t;

int64_t lbbnn_weight_pass_backward_workspace(int O, int I);
int lbbnn_weight_pass_backward(const lbbnn_wpb_args_t* args, void* stream);


/* rng[1] += delta (device side, so graph replays draw fresh noise). */
int lbbnn_rng_advance(uint64_t* rng, uint64_t delta, void* stream);

/* Reproduce the in-kernel N(0,1) draws (tests, and the backward pass that must re-create eps):
 * rows > 0: out[r][c] = normal(counter (row_base + r, c/4))[c%4]  -- lbbnn_lrt_gemm's epilogue indexing;
 * rows == 0: out[i]   = normal(counter (i/4, 0))[i%4], i < cols   -- the 1-D draws of K3 / K5. */
int lbbnn_philox_normal(const uint64_t* rng, uint32_t rng_stream, int64_t row_base, int64_t rows,
                        int64_t cols, float* out, void* stream);

/* log_softmax over the last dim of a (B,O<=64) matrix, in place allowed (…LRT.py:210). */
int lbbnn_log_softmax_rows(const float* in, int ldi, float* out, int ldo, int B, int O, void* stream);

/* Vector-sized backward of one MNF layer with planar flows -- two single-workgroup launches around K1b:
 *
 * lbbnn_mnf_aux_backward: gradient of the KL wrt the auxiliary activations (LBBNN-GP-MF-MNF.py:211-233).
 *   m = mean_o tanh(act_mu + sqrt(act_var)*eps_act);  kl has -log_rb(m; r0_b1, r0_b2, zb_last);
 *   da_mu = g_kl * dkl/dm / O * (1 - act^2),  da_var = da_mu * eps_act / (2 sqrt(act_var));  aux[0] = m.
 *   zb_last = device pointer to scal[3] of the forward.  eps_act == NULL: re-created from the Philox state `rng`
 *   the forward used (stream EPS_ACT of layer_id), as are eps_fwd / eps_kl of the flow backward below.
 *
 * lbbnn_mnf_flow_planar_backward: given dz_fwd / dz_kl (I) from K1b, the upstream g_kl and the column sums of
 *   the output gradients g_sum = sum_b G_m, gv_sum = sum_b G_v (O; gv_sum NULL for a posterior-mean forward), re-runs
 *   the z flow (both draws) and the r flow forward keeping every intermediate z, then walks them backwards
 *   (flows2.py:168-179 planar step; LBBNN-GP-MF-MNF.py:182-187,199-208,224-233) and writes the gradients of
 *   q0_mean, q0_log_var, r0_b1, r0_b2, every flow's u/w/bias, bias_mu and bias_rho.  g_kl NULL = no KL branch
 *   (r-flow / r0_b gradients are then zero-filled).  work: lbbnn_mnf_flow_backward_workspace(I, Tz, Tr) floats.
 */
typedef struct lbbnn_planar_grad {
    float* u[LBBNN_MAX_FLOW_T];
    float* w[LBBNN_MAX_FLOW_T];
    float* b[LBBNN_MAX_FLOW_T];
} lbbnn_planar_grad_t;

typedef struct lbbnn_flow_bwd_args {
    const float *q0_mean, *q0_log_var, *eps_fwd, *eps_kl;   /* (I) */
    const float *r0_b1, *r0_b2;                              /* (I) */
    const float *aux;                                        /* aux[0] = m from lbbnn_mnf_aux_backward      */
    const float *dz_fwd, *dz_kl;                             /* (I) upstream, either may be NULL (= 0)       */
    const float *g_kl;                                       /* device scalar or NULL                        */
    const float *bias_mu, *bias_rho, *g_sum, *gv_sum;        /* (O)                                          */
    lbbnn_planar_flow_t z_flow, r_flow;
    lbbnn_priors_t priors;
    float *d_q0_mean, *d_q0_log_var, *d_r0_b1, *d_r0_b2;     /* (I) outputs                                  */
    float *d_bias_mu, *d_bias_rho;                           /* (O) outputs                                  */
    lbbnn_planar_grad_t d_z_flow, d_r_flow;
    float *work;
    int O, I;
    const uint64_t* rng;                                     /* eps_fwd / eps_kl == NULL: re-create the forward's draws  */
    uint32_t layer_id;                                       /*   (Philox streams EPS_Z / EPS_Z2 of this layer id)       */
} lbbnn_flow_bwd_args_t;

int lbbnn_mnf_aux_backward(const float* act_mu, const float* act_var, const float* eps_act, const float* r0_b1,
                           const float* r0_b2, const float* zb_last, const float* g_kl, int O, int I,
                           float* da_mu, float* da_var, float* aux, const uint64_t* rng, uint32_t layer_id, void* stream);
/* The same for n <= LBBNN_MAX_LAYERS layers in ONE launch (one workgroup per layer).  Every input is a by-product of the
 * forward pass, so a caller that knows d loss / d kl for all layers at once (bnn_amd: the backward of the network's KL sum)
 * runs all of them together. */
typedef struct {
    const float *act_mu, *act_var, *eps_act, *r0_b1, *r0_b2, *zb_last, *g_kl;
    float *da_mu, *da_var, *aux;
    const uint64_t* rng;
    int O, I;
    uint32_t layer_id;
} lbbnn_aux_bwd_args_t;
int lbbnn_mnf_aux_backward_batch(const lbbnn_aux_bwd_args_t* args, int n, void* stream);

/* Gradients of the bias parameters of a layer WITHOUT flows (the LRT layer: BayesianLinear.forward + kl of
 * LBBNN-GP-MF-LRT.py:171-173, 189-196 differentiated by loss.backward(), :223): activation mean + bias_mu, activation variance
 * + softplus(bias_rho)^2, KL bias term.  g_sum / gv_sum (O): column sums of the gradients with respect to the activation
 * mean / variance (lbbnn_output_grad; gv_sum NULL: posterior-mean forward), g_kl: device scalar, the gradient with respect
 * to the layer's KL (NULL: KL not part of the loss).  d_bias_mu = g_sum + g_kl (mu - mu_p) / s_p^2;
 * d_bias_rho = (2 sigma gv_sum + g_kl (sigma / s_p^2 - 1 / sigma)) sigmoid(rho).  Replaces the torch autograd graph over the
 * two bias vectors that the layer's backward built until round 3 (~25 small launches per layer). */
int lbbnn_bias_backward(const float* bias_mu, const float* bias_rho, const float* g_sum, const float* gv_sum,
                        const float* g_kl, const lbbnn_priors_t* priors, float* d_bias_mu, float* d_bias_rho, int O,
                        void* stream);
/* The same from the column-sum PARTIALS that lbbnn_output_grad leaves in its workspace when called with g_sum == NULL (B, O as
 * given there; has_gv: the call had std != NULL): the second level of the sums and the bias gradients in one launch, bitwise
 * what lbbnn_output_grad's own second level followed by lbbnn_bias_backward gives. */
int lbbnn_bias_backward_partials(const float* work, int B, int O, int has_gv, const float* bias_mu, const float* bias_rho,
                                 const float* g_kl, const lbbnn_priors_t* priors, float* d_bias_mu, float* d_bias_rho,
                                 void* stream);
int64_t lbbnn_mnf_flow_backward_workspace(int I, int Tz, int Tr);
int lbbnn_mnf_flow_planar_backward(const lbbnn_flow_bwd_args_t* args, void* stream);
/* The same for n <= LBBNN_MAX_LAYERS layers in ONE launch (one workgroup per layer): the chains are latency-bound and
 * independent of each other, so a network's worth takes the time of one.  Every flow must have at most 4 transforms
 * (LBBNN_E_SHAPE otherwise: use the single-layer entry point).  The caller must have all n layers' inputs ready -- i.e. defer
 * the vector-sized chains to the end of the backward pass (bnn_amd.layers.vector_backward_overlap). */
int lbbnn_mnf_flow_planar_backward_batch(const lbbnn_flow_bwd_args_t* args, int n, void* stream);

/* lbbnn_flow_chain -- a chain of 1-D (vector) flow transforms on one z (I): planar, radial, Householder,
 * Sylvester (flows2.py:72-95, 48-69, 122-135, 98-120) in any order ('mixed' = 5 x (Householder, Planar),
 * flows2.py:31-37).  One single-workgroup launch; fixed-order double-precision block reductions.
 *   z = z_in                                   if z_in != NULL
 *     = q0_mean + exp(q0_log_var)^.5 * eps     otherwise (eps (I) or NULL => Philox stream rng_stream, counter i/4);
 *       log_q0 (if != NULL) = sum(-0.5*log(pi) - 0.5*log_var - 0.5*eps^2-form of LBBNN-GP-MF-MNF.py:213-214)
 *   for each step: z = f(z); logdet += f.log_det()
 * Outputs: z_out (I) (also the working vector; may alias z_in), logdet (1), z_last (1) = z_out[I-1].
 * Step parameters: PLANAR p0=u p1=w p2=bias(1); RADIAL p0=z_0 (I) p1=log_alpha(1) p2=beta(1) -- as written the norm is
 * over the whole vector and H1+H2 is added to every element; HOUSEHOLDER p0=v; SYLVESTER p0=A (I x M row-major)
 * p1=B (M x I) p2=b (M), M <= LBBNN_MAX_SYLVESTER_M, log det by LU with partial pivoting (NaN if det < 0, as torch).
 */
#define LBBNN_FLOW_PLANAR 0
#define LBBNN_FLOW_RADIAL 1
#define LBBNN_FLOW_HOUSEHOLDER 2
#define LBBNN_FLOW_SYLVESTER 3
#define LBBNN_MAX_SYLVESTER_M 8

typedef struct lbbnn_flow_step {
    const float *p0, *p1, *p2;
    int type, M;
} lbbnn_flow_step_t;

typedef struct lbbnn_flow_chain {
    lbbnn_flow_step_t step[LBBNN_MAX_FLOW_T];
    int n;
} lbbnn_flow_chain_t;

int lbbnn_flow_chain(const lbbnn_flow_chain_t* chain, const float* z_in, const float* q0_mean,
                     const float* q0_log_var, const float* eps, const uint64_t* rng, uint32_t rng_stream, int I,
                     float* z_out, float* logdet, float* log_q0, float* z_last, void* stream);
/* The same chain applied to each of the R rows of z_in (R, row stride ldz) independently -- workgroup r carries row r:
 * z_out (R, row stride ldo; may alias z_in), logdet_rows (R, nullable).  This is the row-wise restatement SURVEY.md 8(a) F1
 * defines for a 2-D z (flows2.PropagateFlow itself raises on a 2-D z for planar / Householder / Sylvester / mixed flows:
 * torch.dot, flows2.py:87,129; its Radial transform takes ONE norm over all rows, flows2.py:61 -- not reproduced here). */
int lbbnn_flow_chain_rows(const lbbnn_flow_chain_t* chain, const float* z_in, int ldz, int R, int I,
                          float* z_out, int ldo, float* logdet_rows, void* stream);


/* lbbnn_output_grad -- the (B,O) elementwise head of the layer backward in one pass (LBBNN-GP-MF-LRT.py:172-175 read
 * backwards):   G_m = g_out (.) [out > 0 if relu],   G_v = G_m * eps / (2 std)     (std = sqrt(var_b) of the forward)
 * written both row-major (B,O) -- the A operands of dX = G_m.W_m + 2x(.)(G_v.W_v) -- and transposed (O,B) -- the A
 * operands of dW_m = G_m^T.x, dW_v = G_v^T.x^2 -- plus the column sums g_sum = sum_b G_m, gv_sum = sum_b G_v (the
 * bias gradients).  eps (B,O) explicit, or NULL => re-created in-kernel from the Philox state the forward used
 * (stream rng_stream, counter (row_offset + b, o/4)).  std == NULL => posterior-mean forward: only G_m / G_m^T / g_sum.
 * Column sums are deterministic (per-64-row partials in work, fixed-order second launch).
 */
typedef struct lbbnn_outgrad_args {
    const float *g_out, *out, *std, *eps;     /* (B,O), row strides ldg / ldo / ldo / O; out may be NULL when !relu   */
    const uint64_t* rng;
    float *gm, *gv, *gmT, *gvT;               /* (B,O) dense, (O,B) dense                                              */
    float *g_sum, *gv_sum, *work;             /* (O), (O), lbbnn_output_grad_workspace floats                          */
    int64_t row_offset;
    uint32_t rng_stream;
    int B, O, ldg, ldo, relu;
    const float* gv_scale;                    /* NULL, or (O): G_v[b,o] *= gv_scale[o] -- the variational-dropout alpha
                                                 (d delta / d(x^2 theta^2) = alpha, variational_dropout.py:65)          */
} lbbnn_outgrad_args_t;

int64_t lbbnn_output_grad_workspace(int B, int O);
int lbbnn_output_grad(const lbbnn_outgrad_args_t* args, void* stream);    /* gm == gv == NULL: only the transposes and the sums;
                                                                             g_sum == gv_sum == NULL: the column-sum partials
                                                                             stay in `work` for lbbnn_reduce_partials_batch   */
/* The second level of the two-level column sums of lbbnn_output_grad (Sum_b G_m, Sum_b G_v) and lbbnn_weight_pass_backward
 * (dz_fwd, dz_kl, dr0_c) for SEVERAL layers in one launch: both kernels leave per-row-block partial vectors in their `work`
 * arrays and normally finish them with a launch of their own (six ~5 us launches per training step of a three-layer net);
 * their results are read by the vector-sized backward chains only, so a caller that defers those chains can defer the sums
 * too.  Job: out[q][i] = Sum_b work[b * block_stride + q * q_stride + i], q < nq <= 3, i < ncols, b < nblk, in the order
 * the stand-alone launches use (16 interleaved partial sums over b, added in order): bit-identical results.
 *   lbbnn_output_grad(B, O):              nblk = ceil(B / 64), ncols = O, block_stride = O, q_stride = nblk * O, nq = 1 or 2
 *   lbbnn_weight_pass_backward(O, I):     nblk = ceil(O / 8), ncols = I, ld = (I + 3) & ~3, block_stride = 3 ld, q_stride = ld, nq = 3
 * A NULL out[q] skips that vector.  At most LBBNN_MAX_REDUCE_JOBS jobs per call. */
#define LBBNN_MAX_REDUCE_JOBS 8
typedef struct {
    const float* work;
    float* out[3];
    int64_t block_stride, q_stride;
    int nblk, ncols, nq;
} lbbnn_reduce_job_t;
int lbbnn_reduce_partials_batch(const lbbnn_reduce_job_t* jobs, int n, void* stream);
/* Input gradient of a <= 16-class head in ONE launch: out[b][i] = sum_c gm[b][c] wmT[i][c] + 2 x[b][i] sum_c gv[b][c] wvT[i][c]
 * (gv == wvT == NULL: the first sum alone).  wmT / wvT: [I][ldw] fp32, the (e_w z)^T / var_w^T operands of lbbnn_weight_operands_t. */
int lbbnn_head_dx(const float* gm, const float* gv, int ldg, const float* wmT, const float* wvT, int ldw,
                  const float* x, int ldx, float* out, int ldo, int B, int C, int I, void* stream);
/* Weight gradients of a <= 16-class head as nslabs split-K slabs (lbbnn_weight_pass_backward adds them in order):
 *   dWm[s][c][i] = sum_{b in slab s} gm[b][c] x[b][i],  dWv[s][c][i] = sum_{b in slab s} gv[b][c] x[b][i]^2   ([nslabs][C][I] fp32 each)
 * from the row-major gradients (B,C; row stride ldg) and the row-major layer input (B,I; row stride ldx) -- no transposed
 * operand of x is built (autograd of torch.mm at LBBNN-GP-MF-LRT.py:172-173).  gv == dWv == NULL: the mean product alone.
 * Slab s covers rows [s r, min((s + 1) r, B)), r = ceil(B / nslabs).  Deterministic (fixed order of every addition). */
int lbbnn_head_dw(const float* gm, const float* gv, int ldg, const float* x, int ldx, float* dWm, float* dWv,
                  int B, int C, int I, int nslabs, void* stream);
/* gx (B,I dense) += 2 * x (B,I; row stride ldx) * gxv (B,I dense): the input gradient of the variance GEMM folded
 * into dX = G_m.W_m + 2 x (.) (G_v.W_v)  (d/dx of (x^2).var_w^T, LBBNN-GP-MF-LRT.py:173). */
/* out = comb_add + 2 * comb_x (.) (x . w_op^T): the mean-only product of lbbnn_lrt_gemm with lbbnn_dx_combine fused into
 * its epilogue -- dX = G_m.W_m + 2 x (.) (G_v.W_v) is the second product's output directly (comb_add = G_m.W_m,
 * comb_x = the layer input).  comb_x / comb_add: (B,O) with row strides ld_cx / ld_ca; out may alias comb_add.
 * O > 16 (LBBNN_E_SHAPE otherwise); flags: LBBNN_F_SPLIT16 as for lbbnn_lrt_gemm. */
int lbbnn_lrt_gemm_combine(const float* x, int ldx, const void* w_op, int ld, const float* comb_x, int ld_cx,
                           const float* comb_add, int ld_ca, float* out, int ldo, int B, int I, int O, int flags,
                           void* stream);
int lbbnn_dx_combine(float* gx, const float* gxv, const float* x, int ldx, int B, int I, void* stream);

/* lbbnn_adam_step -- torch.optim.Adam's update (the optimizer of the reference's training scripts,
 * LBBNN-GP-MF-LRT.py:358, LBBNN-GP-MF-MNF.py:421) for a LIST of parameter tensors in one launch:
 *   g' = g + weight_decay * p;  m = b1 m + (1-b1) g';  v = b2 v + (1-b2) g'^2;  t = *step + 1
 *   p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
 * *step is a device-side float counter, read by every workgroup; advance != 0 adds 1 to it in a second one-thread
 * launch (set it on the last list of an optimizer step), so the whole step is HIP-graph capturable.
 */
#define LBBNN_ADAM_MAX_TENSORS 80
typedef struct lbbnn_adam_list {
    float* p[LBBNN_ADAM_MAX_TENSORS];
    const float* g[LBBNN_ADAM_MAX_TENSORS];
    float* m[LBBNN_ADAM_MAX_TENSORS];
    float* v[LBBNN_ADAM_MAX_TENSORS];
    int64_t numel[LBBNN_ADAM_MAX_TENSORS];
    int n;
} lbbnn_adam_list_t;

int lbbnn_adam_step(const lbbnn_adam_list_t* list, float lr, float beta1, float beta2, float eps, float weight_decay,
                    float* step, int advance, void* stream);

/* lbbnn_adam_step_groups -- the same update for a list of tensors that belong to ANY NUMBER of parameter groups, in ONE
 * launch (the reference's baseline optimizer has 33 single-tensor groups with four rates, LBBNN-GP-MF.py:520-554).
 * Nothing a scheduler may change is a kernel argument: tensor i reads row group[i] of `hyper`, a DEVICE table of n_groups
 * rows, when the kernel runs, so a captured graph follows the table (lr decay, freezing a group with lr = 0) without a
 * re-capture.  Per element, with h = hyper[group[i]] and t = step[group[i]] + 1:
 *   g' = g;  mask[i] != NULL: g' = g' * mask[i][e] (COND_OPT, LBBNN-GP-MF.py:333-336);  grad_scale != NULL: g' = g' * *grad_scale
 *   LBBNN_ADAM_F_DECOUPLED: p = p * (1 - h.lr * h.weight_decay), then the update with weight_decay = 0 (AdamW)
 *   otherwise lbbnn_adam_step's update, expression for expression: without mask, scale and decoupled decay the results
 *   are bitwise those of lbbnn_adam_step with the same five values.
 * step: n_groups device-side float counters, one per group, contiguous.  advance != 0 (set it on the last list of an
 * optimizer step): every group without LBBNN_ADAM_F_INACTIVE gets step[g] += 1, IN THE SAME LAUNCH, by the workgroup that
 * finishes last (a ticket drawn from *ticket after the workgroup's last use of its counter; DESIGN.md 9.1 has the argument
 * why no workgroup can read an advanced counter).  ticket: one device uint32 the caller zeroes ONCE; the last workgroup
 * leaves it at zero again.  One optimizer may have one such launch in flight at a time (launches of one stream are).
 * list->n == 0 with advance != 0 is a one-workgroup launch that only advances.  Launches: exactly 1.
 * Checks (before any HIP call): list / hyper / step, ticket with advance, a tensor's p / g / m / v: LBBNN_E_NULL;
 * n outside [0, LBBNN_ADAM_GROUPS_MAX_TENSORS], n_groups outside [1, 65536], numel <= 0, group[i] outside [0, n_groups):
 * LBBNN_E_SHAPE.  The list goes by value in the kernel arguments (4 KiB segment), hence the lower tensor limit. */
#define LBBNN_ADAM_GROUPS_MAX_TENSORS 64
#define LBBNN_ADAM_CHUNK 4096          /* elements per workgroup of the list kernels = per partial of lbbnn_grad_sumsq */
#define LBBNN_ADAM_F_DECOUPLED 0x1     /* decoupled weight decay (torch.optim.AdamW)                     */
#define LBBNN_ADAM_F_INACTIVE 0x2      /* a group without parameters: its counter does not advance       */
typedef struct lbbnn_adam_hyper {      /* one row of the device table; 24 bytes                          */
    float lr, beta1, beta2, eps, weight_decay;
    uint32_t flags;
} lbbnn_adam_hyper_t;
typedef struct lbbnn_adam_group_list {
    float* p[LBBNN_ADAM_GROUPS_MAX_TENSORS];
    const float* g[LBBNN_ADAM_GROUPS_MAX_TENSORS];
    float* m[LBBNN_ADAM_GROUPS_MAX_TENSORS];
    float* v[LBBNN_ADAM_GROUPS_MAX_TENSORS];
    const float* mask[LBBNN_ADAM_GROUPS_MAX_TENSORS];   /* same shape as g; NULL = no mask */
    int64_t numel[LBBNN_ADAM_GROUPS_MAX_TENSORS];
    int group[LBBNN_ADAM_GROUPS_MAX_TENSORS];
    int n;
} lbbnn_adam_group_list_t;

int lbbnn_adam_step_groups(const lbbnn_adam_group_list_t* list, const lbbnn_adam_hyper_t* hyper, float* step, int n_groups,
                           const float* grad_scale, uint32_t* ticket, int advance, void* stream);

/* lbbnn_sgd_step_groups -- torch.optim.SGD's update (the optimizer of the baseline simulation study: eleven single-tensor
 * groups at two rates, six of them set to 0 at epoch 50, LBBNN-GP-MFsim_study.py) in the form of lbbnn_adam_step_groups: a
 * list of tensors of ANY NUMBER of parameter groups in ONE launch, every value a schedule may change read from a DEVICE table
 * when the kernel runs.  The list is lbbnn_adam_group_list_t (so lbbnn_grad_sumsq gives the clipping scale unchanged): m[i] is
 * the momentum buffer, NULL = no momentum for that tensor; v is not read and may be NULL.  Per element, with
 * h = hyper[group[i]] and t = step[group[i]]:
 *   g' = g;  mask[i] != NULL: g' = g' * mask[i][e];  grad_scale != NULL: g' = g' * *grad_scale
 *   h.weight_decay != 0: g' = g' + h.weight_decay * p
 *   m[i] != NULL and h.momentum != 0:  buf = (t == 0) ? g' : h.momentum * buf + (1 - h.dampening) * g'  (stored; the first step
 *       does not read the buffer);  g' = LBBNN_SGD_F_NESTEROV ? g' + h.momentum * buf : buf
 *   p = p - h.lr * g'
 * The "first step" is per GROUP (t == 0), where torch keeps it per parameter: a parameter that receives its first gradient
 * later than its group differs from torch only when dampening != 0.
 * step / ticket / advance: as lbbnn_adam_step_groups, the same device code (every group without LBBNN_SGD_F_INACTIVE gets
 * step[g] += 1 in the same launch, by the workgroup that finishes last).  list->n == 0 with advance != 0 is a
 * one-workgroup launch that only advances.  Launches: exactly 1.
 * Checks (before any HIP call): list / hyper / step, ticket with advance, a tensor's p / g: LBBNN_E_NULL; n outside [0,
 * LBBNN_ADAM_GROUPS_MAX_TENSORS], n_groups outside [1, 65536], numel <= 0, group[i] outside [0, n_groups): LBBNN_E_SHAPE. */
#define LBBNN_SGD_F_NESTEROV 0x1       /* Nesterov momentum                                              */
#define LBBNN_SGD_F_INACTIVE 0x2       /* a group without parameters: its counter does not advance       */
typedef struct lbbnn_sgd_hyper {       /* one row of the device table; 20 bytes                          */
    float lr, momentum, dampening, weight_decay;
    uint32_t flags;
} lbbnn_sgd_hyper_t;

int lbbnn_sgd_step_groups(const lbbnn_adam_group_list_t* list, const lbbnn_sgd_hyper_t* hyper, float* step, int n_groups,
                          const float* grad_scale, uint32_t* ticket, int advance, void* stream);

/* lbbnn_adam_step_groups_guarded / lbbnn_sgd_step_groups_guarded -- the two list steps above behind a device-side guard: the
 * found-inf flag of a training step that the host never looks at (a replayed graph).  Every workgroup reads, once, at its entry,
 *   skip = (*guard != 0) || (grad_scale != NULL && !isfinite(*grad_scale))
 * guard: one device int32, e.g. the word lbbnn_elbo_loss_monitor writes; the second term makes clipping a gradient check
 * (lbbnn_grad_sumsq leaves a NaN scale for a NaN or infinite norm; max_norm = inf gives a scale of exactly 1 otherwise).
 * skip == 0: the same device code as the unguarded entry point, bitwise its result.
 * skip != 0: no workgroup reads or writes p, m or v; with advance != 0 the workgroup that finishes last does NOT advance the
 *   counters, adds 1 to *skipped (int64, nullable; a plain read-modify-write by one thread: launches of one stream are ordered)
 *   and leaves the ticket at zero as always.  A step of several lists reads the same two words in every launch and counts the
 *   skip once, in the launch with advance != 0.
 * Both words are written by earlier launches of the stream and by nothing in this launch, so every workgroup sees the same
 * value whenever it runs.  One launch per call, as for the unguarded entry points.
 * Checks (before any HIP call): those of the unguarded entry point, and guard NULL: LBBNN_E_NULL. */
int lbbnn_adam_step_groups_guarded(const lbbnn_adam_group_list_t* list, const lbbnn_adam_hyper_t* hyper, float* step, int n_groups,
                                   const float* grad_scale, uint32_t* ticket, int advance, const int32_t* guard, int64_t* skipped,
                                   void* stream);
int lbbnn_sgd_step_groups_guarded(const lbbnn_adam_group_list_t* list, const lbbnn_sgd_hyper_t* hyper, float* step, int n_groups,
                                  const float* grad_scale, uint32_t* ticket, int advance, const int32_t* guard, int64_t* skipped,
                                  void* stream);

/* lbbnn_grad_sumsq -- global L2 norm of the (masked) gradients of a list, for torch.nn.utils.clip_grad_norm_'s clipping
 * applied inside lbbnn_adam_step_groups (p / m / v / group of the list are not read).  Launch 1: workgroup b of the list
 * (tensor i owns ceil(numel[i] / LBBNN_ADAM_CHUNK) consecutive workgroups, tensors in list order) writes
 * work[work_offset + b] = sum over its chunk of (mask * g)^2, added in a fixed order.  finalize_count > 0 (set it on the last
 * list of a step, to the number of partials of all its lists) adds launch 2, one workgroup: the partials work[0 ..
 * finalize_count) are summed in the fixed order of the project's two-level column sums (64 columns, every 16th row per wave,
 * then the 16 wave partials, then the 64 columns by a fixed butterfly), and
 *   *norm = sqrt(sum),  *grad_scale = min(1, max_norm / (*norm + 1e-6))      (clip_grad_norm_'s formula; a NaN norm gives NaN)
 * No atomics: *norm is bitwise reproducible from run to run.  Launches: 1, or 2 with finalize_count > 0.
 * work: lbbnn_grad_sumsq_workspace(partials of all lists) floats (the partials padded to a multiple of 64, plus 64).
 * Checks: list / work, norm / grad_scale with finalize_count > 0, a tensor's g: LBBNN_E_NULL; n outside [0,
 * LBBNN_ADAM_GROUPS_MAX_TENSORS], numel <= 0, work_offset < 0, finalize_count < 0, and with finalize_count > 0: finalize_count !=
 * work_offset + this list's partials (the zero padding is written behind the last list), max_norm <= 0: LBBNN_E_SHAPE. */
int64_t lbbnn_grad_sumsq_workspace(int64_t partials);
int lbbnn_grad_sumsq(const lbbnn_adam_group_list_t* list, float* work, int64_t work_offset, int64_t finalize_count,
                     float max_norm, float* norm, float* grad_scale, void* stream);

/* lbbnn_matmul_splitk -- split-K form of the mean-only bf16x3 product for long contractions with few output tiles
 * (the weight gradients dW = G^T.x: K = batch):  out[z] (B,O; row stride ldo; slab stride B*ldo) =
 * x[:, Kz] . w[:, Kz]^T with Kz = [z*kchunk, min(I, (z+1)*kchunk)), z < ceil(I / kchunk); kchunk a multiple of 32.
 * w_op: LBBNN_F_SPLIT16 operand of lbbnn_transpose_operand / lbbnn_weight_pass.  The consumer adds the slabs
 * (lbbnn_weight_pass_backward does, in a fixed order => deterministic).
 */
int lbbnn_matmul_splitk(const float* x, int ldx, const void* w_op, int ld, float* out, int ldo,
                        int B, int I, int O, int kchunk, void* stream);

/* lbbnn_multi_copy -- dst[i][0..numel[i]) = src[i][...] for a LIST of fp32 tensors in one launch: packing the gradients
 * of all parameters into the flat bucket that is all-reduced over RCCL (and unpacking it), instead of one copy kernel
 * per parameter tensor. */
typedef struct lbbnn_copy_list {
    float* dst[LBBNN_ADAM_MAX_TENSORS];
    const float* src[LBBNN_ADAM_MAX_TENSORS];      /* NULL = fill dst with zeros (a parameter without a gradient) */
    int64_t numel[LBBNN_ADAM_MAX_TENSORS];
    int n;
} lbbnn_copy_list_t;

int lbbnn_multi_copy(const lbbnn_copy_list_t* list, void* stream);

/* Stand-alone application of a dense coupling flow (RNVP / MNF type, flows2.py:188-241) to ONE vector, and its analytic
 * backward -- the pieces the vector-sized backward of an MNF layer with the reference's default flows is made of:
 *   lbbnn_flow_dense_apply:           z_out = f_T(...f_1(z_in)),  *logdet = sum of the transforms' log-dets
 *   lbbnn_flow_dense_apply_backward:  given d_zout (I) and *d_logdet (device scalar, NULL = 0): dz_in (I) and the
 *                                     gradient of every parameter of every transform (written, not accumulated).
 * which_mask selects mask_fwd (0) or mask_kl (1) of each transform.  One single-workgroup launch each; the backward
 * re-runs the forward keeping each transform's input (work: lbbnn_flow_dense_apply_workspace floats).
 */
#define LBBNN_MAX_DENSE_T 8
typedef struct lbbnn_dense_grad {
    float *w_in, *b_in, *w_mid[3], *b_mid[3], *w_a, *b_a, *w_b, *b_b;      /* same shapes as lbbnn_dense_transform_t */
} lbbnn_dense_grad_t;

int64_t lbbnn_flow_dense_apply_workspace(int I, int T);
int lbbnn_flow_dense_apply(const lbbnn_dense_transform_t* tr, int T, int which_mask, const float* z_in, int I,
                           float* z_out, float* logdet, void* stream);
int lbbnn_flow_dense_apply_backward(const lbbnn_dense_transform_t* tr, const lbbnn_dense_grad_t* grads, int T,
                                    int which_mask, const float* z_in, const float* d_zout, const float* d_logdet, int I,
                                    float* dz_in, float* work, void* stream);

/* lbbnn_flow_dense_rows -- the same coupling flows applied to R ROWS at once (each row with its own Bernoulli mask per
 * transform), the dense affine steps on the matrix cores (v_mfma_f32_16x16x4_f32, exact fp32).  This is the as-written form
 * of `sample_z(batch_size)` (LBBNN-GP-MF-MNF.py:182-187: z_flow on a (B,I) matrix of which only the last row is kept -- the
 * layer kernels above compute that row alone) and what the stand-alone `PropagateFlow('RNVP'|'MNF').forward(z)` of
 * flows2.py:41-46,206-219,233-241 computes for a 1-D or (R,I) z.
 *   z_out (R, row stride ldo)  = f_T(... f_1(z_in))  row by row; may alias z_in
 *   logdet_rows (R), nullable  = sum_t sum_i (1 - m) log gate   (RNVP's log_det is this per-row vector, flows2.py:218-219;
 *                                the MNF type's is its sum over ALL rows, flows2.py:240-241: the caller adds the R values)
 *   masks [T][R][I] in {0,1}, or NULL: Bernoulli(0.5) drawn in-kernel from Philox (rng = {seed, offset}, stream
 *   rng_stream, counter = (row_base + row, t, i/4)); mask_out (nullable, [T][R][I]) receives the masks used.
 * The mask_fwd / mask_kl fields of the transforms are ignored.  One launch: a 256-thread workgroup carries 16 rows through
 * the whole chain with z resident in LDS.  I <= lbbnn_flow_dense_rows_max_dim() (LDS capacity; LBBNN_E_SHAPE otherwise).
 * Deterministic (fixed-order sums, no atomics). */
/* lbbnn_q0_rows -- the R-row z0 of sample_z(batch_size = R) (LBBNN-GP-MF-MNF.py:183-185):
 *   z0[r][i] = q0_mean[i] + exp(q0_log_var[i])^(1/2) * eps[r][i],   z0 (R,I) dense rows
 * eps (R,I) explicit, or NULL: N(0,1) from Philox stream rng_stream with counter (i/4, R-1-r) -- the last row's draw is
 * the draw the fused layer kernels make for the kept row, so both forms see the same z there. */
int lbbnn_q0_rows(const float* q0_mean, const float* q0_log_var, const float* eps, const uint64_t* rng,
                  uint32_t rng_stream, int R, int I, float* z0, void* stream);
int lbbnn_flow_dense_rows_max_dim(void);
int lbbnn_flow_dense_rows(const lbbnn_dense_transform_t* tr, int T, const float* masks, float* mask_out,
                          const uint64_t* rng, uint32_t rng_stream, uint64_t row_base,
                          const float* z_in, int ldz, int R, int I,
                          float* z_out, int ldo, float* logdet_rows, void* stream);

/* lbbnn_mnf_flow_dense_backward -- the vector-sized backward (cf. lbbnn_mnf_flow_planar_backward) for a layer whose flows are dense coupling flows
 * (RNVP / MNF type, flows2.py:188-241; the reference's default).  Inputs as lbbnn_mnf_flow_planar_backward; the
 * transforms (with the masks of the forward call) in zt / rt, their gradient destinations in d_zt / d_rt (host arrays),
 * and `save` = what the forward kept (lbbnn_dense_layer_t::save).  2 + 3*(Tz+Tr) launches spread over workgroups: per
 * transform, walking backwards, the two I x H heads (outer-product gradients, share of dy), the H x H chain in one
 * workgroup, the H x I input layer.  Both draws of the z flow are handled together and the SUM of their parameter
 * gradients is written once; every reduction has a fixed order (deterministic).  g_kl NULL: no KL branch, r-flow and
 * r0_b gradients are zero-filled.  Tz / Tr must be the values the forward ran with (they fix the layout of `save`).
 * work: lbbnn_mnf_flow_dense_backward_workspace(I) floats.
 */
typedef struct lbbnn_dense_bwd_args {
    const float *q0_mean, *q0_log_var, *eps_fwd, *eps_kl;   /* (I); eps NULL: re-created from rng / layer_id          */
    const float *r0_b1, *r0_b2;                              /* (I)                                                   */
    const float *aux;                                        /* aux[0] = m from lbbnn_mnf_aux_backward                */
    const float *dz_fwd, *dz_kl;                             /* (I) upstream from K1b, either may be NULL (= 0)       */
    const float *g_kl;                                       /* device scalar or NULL                                 */
    const float *bias_mu, *bias_rho, *g_sum, *gv_sum;        /* (O)                                                   */
    const lbbnn_dense_transform_t *zt, *rt;
    const lbbnn_dense_grad_t *d_zt, *d_rt;
    lbbnn_priors_t priors;
    float *d_q0_mean, *d_q0_log_var, *d_r0_b1, *d_r0_b2;     /* (I) outputs                                           */
    float *d_bias_mu, *d_bias_rho;                           /* (O) outputs                                           */
    const float *save;
    float *work;
    int Tz, Tr, O, I;
    const uint64_t* rng;
    uint32_t layer_id;
} lbbnn_dense_bwd_args_t;

int64_t lbbnn_mnf_flow_dense_backward_workspace(int I);
int lbbnn_mnf_flow_dense_backward(const lbbnn_dense_bwd_args_t* args, void* stream);
/* n <= LBBNN_MAX_LAYERS layers in the SAME 2 + 3*(Tz+Tr) launches (blockIdx.z = layer): the launches are latency-bound, so a
 * network's worth takes about the time of one layer.  The layers must agree on Tz, Tr and on having a KL branch
 * (LBBNN_E_SHAPE otherwise), and all of their inputs must be ready: defer the chains to the end of the backward pass. */
int lbbnn_mnf_flow_dense_backward_batch(const lbbnn_dense_bwd_args_t* args, int n, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The descriptor form of the dual-moment GEMM (every operand format), and round 3's row-scaled FP16 operand format
 * (LBBNN_F_F16S), which only the descriptor form takes.
 *
 * lbbnn_lrt_gemm is the product and nothing else.  lbbnn_lrt_gemm_ex(desc) carries everything a forward adds to it:
 *   - std_out (refused together with LBBNN_F_MEAN_ONLY: LBBNN_E_FLAGS);
 *   - layers / n_layers / fin_rng / kl_total: the work of lbbnn_layers_finalize for the n_layers layers (every layer's KL tail
 *     from its descriptor, kl_layer outputs, *kl_total if non-NULL), computed by ONE extra workgroup of the same launch while
 *     the tiles are computed: the KL tail depends on parameters only, so it needs no launch of its own.  fin_rng: the state K5
 *     draws eps_act from (rng_snap of lbbnn_layers_operands_snap).  When the kernel selected for this shape cannot host the
 *     extra workgroup (small-tile configuration, O <= 16, not enough dynamic LDS) the finalize runs as a launch of its own
 *     after the GEMM: same results either way.  n_layers = 0 is the plain product;
 *   - rng_live / advance: rng_live[1] += advance, done by the same extra workgroup (with n_layers = 0: a tiny launch after
 *     the GEMM);
 *   - with LBBNN_F_F16S: x as planes, planes out, the head fold.
 * Flags by format.  Without LBBNN_F_F16S (fp32 rows, or bf16 hi | lo with LBBNN_F_SPLIT16): the flags and checks of
 * lbbnn_lrt_gemm; LBBNN_F_VAR1, LBBNN_F_XPLANES or a non-NULL mean_scale, wvar_scale, out_planes or head_out is refused with
 * LBBNN_E_FLAGS before anything else is looked at.  With LBBNN_F_F16S: LBBNN_F_RELU | LBBNN_F_VAR1 | LBBNN_F_XPLANES only.
 *
 * Arithmetic (replaces the same reference lines as lbbnn_lrt_gemm: LBBNN-GP-MF-LRT.py:172-175, LBBNN-GP-MF-MNF.py:197-200):
 *   every operand value w is held as hi + lo, both IEEE fp16, products on v_mfma_f32_16x16x32_f16, fp32 accumulate:
 *     mean = x.e_w^T    as xh.eh + xh.el + xl.eh                      (the dropped xl.el term is 2^-22 relative)
 *     var  = x^2.var_w^T as sh.vh + sh.vl + sl.vh, s = x^2 * 2^-8     (LBBNN_F_VAR1: sh.vh alone, sh = RNE16(s))
 *   fp16 has 5 exponent bits, so the weight operands carry one exact power-of-two scale per output row (e_scale[o],
 *   v_scale[o]: the row maximum lands in [2^13, 2^14)) which the epilogue takes out of the accumulators again, and x^2 is
 *   formed from x * 2^-4 (fp16 overflows at 65504: the format holds |x| < 4096; a producer that sees a larger activation
 *   poisons its output with NaN rather than saturating silently -- `range_guard`).
 *   Measured against fp64 on the headline layers (tools/format_error.py): 3 + 3 products 2.3-3.0e-8 of max|out| (an fp32
 *   accumulate of exact products, torch.mm, gives 1-3e-7), 3 + 1 products 1.4-1.8e-5 (contract: 1e-4).
 *
 * Layout: a weight row is the 128-B-line form of LBBNN_F_SPLIT16 (lbbnn_device.h) with fp16 values.  x may be given
 *   - as fp32 rows (the network input): split in registers by the consumer, or
 *   - as PLANES (LBBNN_F_XPLANES): rows of ldx fp32-sized slots, per 32-k chunk one 128-B line of units
 *     (xh k0-7 | xl k0-7 | xh k8-15 | xl k8-15 | ...), ldx a multiple of 32, tail k >= I zero -- what this GEMM writes
 *     to `out_planes` for the next layer (ReLU applied) and what lbbnn_format_x makes from fp32 rows.  A consumer of
 *     planes spends 4 packed-fp16 instructions per 2 k on x^2 and none on the split.
 */
#define LBBNN_F_F16S 0x40      /* operands in the row-scaled fp16 hi + lo format (mean_scale / wvar_scale required) */
#define LBBNN_F_VAR1 0x80      /* with LBBNN_F_F16S: ONE product for the variance GEMM (3 + 1 products per tile step); var_w is then a
                                  plain fp16 matrix [O][ld] halves (the hi part alone: 64 B per row and K step instead of 128)  */
#define LBBNN_F_XPLANES 0x100  /* with LBBNN_F_F16S: x is given as fp16 hi | lo planes                                */

typedef struct lbbnn_gemm_desc {
    const void* x; int ldx;                      /* (B, I): fp32 rows of ldx floats, or planes (ldx fp32-sized slots per row) */
    const void* e_w; const void* var_w; int ld;  /* [O][ld] operands in the format `flags` names (lbbnn_layers_operands, lbbnn_weight_pass[_f16]) */
    const float* mean_scale;                     /* (O) e_scale; NULL without LBBNN_F_F16S */
    const float* wvar_scale;                     /* (O) v_scale; NULL without LBBNN_F_F16S */
    const float* bias_mean;                      /* (O) or NULL  */
    const float* bias_var;                       /* (O) or NULL  */
    const float* var_scale;                      /* (O) or NULL: extra per-feature factor on the variance product */
    const float* eps;                            /* (B, O) explicit N(0,1) draws, or NULL => Philox(rng)          */
    const uint64_t* rng; uint32_t rng_stream; int64_t row_offset;
    float* out; int ldo;                         /* (B, O) fp32 output, or NULL when only planes are wanted       */
    void* out_planes; int ldp;                   /* (B, ldp) plane rows for the next layer, or NULL; needs O % 8 == 0, ldp % 32 == 0 */
    float* std_out;                              /* (B, O) sqrt(var) for the backward pass, or NULL               */
    int B, I, O, flags;                          /* LBBNN_F_F16S with LBBNN_F_RELU | LBBNN_F_VAR1 | LBBNN_F_XPLANES, or the flags of lbbnn_lrt_gemm */
    /* optional KL finalize of a network and RNG advance carried by one extra workgroup (above) */
    const lbbnn_layer_desc_t* layers; int n_layers; const uint64_t* fin_rng; float* kl_total;
    uint64_t* rng_live; uint64_t advance;
    /* optional HEAD FOLD (head_out != NULL; needs LBBNN_F_RELU): the layer that FOLLOWS this one has head_classes <= 16 outputs
     * (the 10-class head of BayesianNetwork, LBBNN-GP-MF-MNF.py:255-256).  Its two moment products are formed in this launch's
     * epilogue from the accumulators (fp16 hi + lo on v_mfma_f32_16x16x16_f16, per-o-tile partials in head_slab), a second small
     * launch adds the partials, the head's bias / variance bias / noise (head_eps or Philox(rng, head_rng_stream)) and, with
     * LBBNN_F_LOG_SOFTMAX in head_flags, log_softmax: head_out (B, head_classes).  head_e / head_v: the head's fp32 operands
     * [head_classes][head_ld] (lbbnn_layers_operands, split == 0).  `out` / `out_planes` may then both be NULL: the hidden
     * activation of this layer is never stored.  head_slab: lbbnn_head_slab_floats(B, O) floats. */
    const float* head_e; const float* head_v; int head_ld; int head_classes;
    const float* head_bias_mean; const float* head_bias_var; const float* head_eps; uint32_t head_rng_stream;
    float* head_out; int head_ldo; float* head_slab; int head_flags;
} lbbnn_gemm_desc_t;

int lbbnn_lrt_gemm_ex(const lbbnn_gemm_desc_t* d, void* stream);
int64_t lbbnn_head_slab_floats(int B, int O);

/* fp32 rows -> fp16 hi | lo planes (the x format above); I % 8 == 0, x 16-B aligned rows, ldp % 32 == 0, ldp >= I.
 * Writes the whole row of planes (tail slots zero). */
int lbbnn_format_x(const float* x, int ldx, void* planes, int ldp, int B, int I, void* stream);

/* The scalar head of the training step (train(), LBBNN-GP-MF-MNF.py:268-271), one launch each, deterministic:
 *   lbbnn_elbo_loss:            *loss = -sum_b logp[b][target[b]] + (kl ? *kl * kl_scale : 0)   (F.nll_loss(reduction='sum') + kl / N)
 *   lbbnn_elbo_loss_backward:   g_logp[b][c] = -(*g) (c == target[b]);  *g_kl = (*g) * kl_scale (g_kl may be NULL)
 *   lbbnn_log_softmax_backward: out = g - exp(logp) * rowsum(g)   (backward of F.log_softmax(dim=1), C <= 64)
 * target: int64 class indices (entries outside [0, C) contribute nothing, as ignore_index does). */
int lbbnn_elbo_loss(const float* logp, int ldp, const int64_t* target, int B, int C, const float* kl, float kl_scale,
                    float* loss, void* stream);
int lbbnn_elbo_loss_backward(const float* g, const int64_t* target, int B, int C, float kl_scale, float* g_logp, float* g_kl,
                             void* stream);
/* lbbnn_elbo_loss_monitor -- lbbnn_elbo_loss with the running totals of a training log and a per-step "loss is not finite"
 * flag, in the SAME single launch of one workgroup.  *loss is bitwise what lbbnn_elbo_loss writes for the same arguments (the
 * same terms, added in the same order).  The backward launches are lbbnn_elbo_loss_backward[_logits], unchanged.
 * totals: LBBNN_MONITOR_WORDS device int64 words that every call ADDS to (the caller zeroes them); LBBNN_MONITOR_COUNTS counts,
 * then LBBNN_MONITOR_SUMS doubles stored as their bit patterns.  Counts, at these indices:
 *   LBBNN_MONITOR_STEPS            calls
 *   LBBNN_MONITOR_ROWS             B
 *   LBBNN_MONITOR_CORRECT          rows with a valid target whose arg-max over the C log-probabilities equals it, by
 *                                  numpy.argmax's rule: a NaN compares as the maximum, the lowest index of the maximum wins
 *   LBBNN_MONITOR_BAD_TARGETS      rows with target < 0 or >= C (no loss term, no gradient, not in `correct`)
 *   LBBNN_MONITOR_NONFINITE_ROWS   rows whose C log-probabilities are not all finite
 *   LBBNN_MONITOR_NONFINITE_STEPS  calls whose *loss is inf or NaN
 *   LBBNN_MONITOR_SKIPPED_STEPS    not written here: the slot the guarded optimizer steps count in (`skipped`, below)
 *   LBBNN_MONITOR_NLL_ROWS         rows with a valid target of the calls whose *loss is finite: what nll_sum is a sum over
 * Sums (index LBBNN_MONITOR_COUNTS + ...), with nll = -sum_b logp[b][target[b]] and kl_term = kl ? *kl * kl_scale : 0 in fp64:
 *   LBBNN_MONITOR_NLL_SUM, LBBNN_MONITOR_KL_TERM_SUM, LBBNN_MONITOR_LOSS_SUM   += nll, kl_term, nll + kl_term -- ONLY on a call
 *                                  whose *loss is finite, so that one bad batch does not destroy the means of an epoch
 *   LBBNN_MONITOR_LAST_NLL, LBBNN_MONITOR_LAST_LOSS   overwritten by every call: nll, and (double)*loss -- what train() prints
 * guard (nullable): one device int32, OVERWRITTEN by every call: 1 when *loss is not finite, else 0 (per step, not sticky).
 * One workgroup and the order of a stream's launches make plain read-modify-writes by one thread enough: no atomics, every
 * total the same bits from run to run.  One monitor may have one such launch in flight at a time (launches of one stream are).
 * Checks (before any HIP call): logp / target / loss / totals NULL: LBBNN_E_NULL; B <= 0, C <= 0, C > 64, ldp < C:
 * LBBNN_E_SHAPE.  kl and guard are nullable. */
#define LBBNN_MONITOR_COUNTS 8
#define LBBNN_MONITOR_STEPS 0
#define LBBNN_MONITOR_ROWS 1
#define LBBNN_MONITOR_CORRECT 2
#define LBBNN_MONITOR_BAD_TARGETS 3
#define LBBNN_MONITOR_NONFINITE_ROWS 4
#define LBBNN_MONITOR_NONFINITE_STEPS 5
#define LBBNN_MONITOR_SKIPPED_STEPS 6
#define LBBNN_MONITOR_NLL_ROWS 7
#define LBBNN_MONITOR_SUMS 5
#define LBBNN_MONITOR_NLL_SUM 0
#define LBBNN_MONITOR_KL_TERM_SUM 1
#define LBBNN_MONITOR_LOSS_SUM 2
#define LBBNN_MONITOR_LAST_NLL 3
#define LBBNN_MONITOR_LAST_LOSS 4
#define LBBNN_MONITOR_WORDS (LBBNN_MONITOR_COUNTS + LBBNN_MONITOR_SUMS)
int lbbnn_elbo_loss_monitor(const float* logp, int ldp, const int64_t* target, int B, int C, const float* kl, float kl_scale,
                            float* loss, int64_t* totals, int32_t* guard, void* stream);
/* lbbnn_elbo_loss_backward and, in the same launch, the gradient with respect to the LOGITS when `logp` is the log_softmax of a
 * layer's logits (what lbbnn_log_softmax_backward would make of g_logp: bitwise the same): g_logits (B,C dense). */
int lbbnn_elbo_loss_backward_logits(const float* g, const int64_t* target, const float* logp, int ldp, int B, int C,
                                    float kl_scale, float* g_logp, float* g_logits, float* g_kl, void* stream);
int lbbnn_log_softmax_backward(const float* g, int ldg, const float* logp, int ldp, float* out, int ldo, int B, int C,
                               void* stream);

/* The binary (sigmoid) head and its fused loss: torch.sigmoid on the last layer's logits and nn.BCELoss(reduction='sum') +
 * kl / NUM_BATCHES, the logistic-regression form of the networks.  One launch each, one pass, fixed-order sums, no atomics:
 * the same bits from run to run.  (B, O) blocks with dense rows and a free row stride (ld*, floats); 0 <= B, 1 <= O <= 16,
 * B * O < 2^31, every ld >= O (LBBNN_E_SHAPE); a required pointer NULL: LBBNN_E_NULL; a pointer off 4 bytes: LBBNN_E_ALIGN.
 *
 * lbbnn_binary_head: probs[b][o] = 1 / (1 + expf(-x)) (may be `logits` itself: in place) and / or, for O == 1 only
 *   (LBBNN_E_SHAPE otherwise; ld2 >= 2), logp2 (B, 2) = [logsigmoid(-x), logsigmoid(x)] with logsigmoid(x) = min(x, 0) -
 *   log1pf(expf(-|x|)): the log-probabilities of the two classes, formed from the logit (finite for every finite x; log(1 - p)
 *   would be -inf from x = 17 on).  Either output may be NULL, not both (LBBNN_E_NULL).  B == 0: a successful no-op.  A member
 *   dimension is the caller's: (S, B, O) dense is B' = S * B, padded members are one call each.
 * lbbnn_elbo_bce_loss: one workgroup, fp64 partial sums:
 *   *loss = sum_{b,o} ( (y - 1) max(log1pf(-p), -100) - y max(logf(p), -100) ) + (kl ? *kl * kl_scale : 0)
 *   -- -(y log p + (1 - y) log(1 - p)) in the spelling of torch's binary_cross_entropy (its fp32 terms up to the last bit of
 *   logf, which is not torch.log's on every input; log1pf agrees with torch.log1p).
 *   target: fp32 in [0, 1], the shape of probs.  stats (int32[4], nullable; accumulate != 0 adds to what it holds):
 *     [0] correct          elements with a valid target and (p > 0.5f) == (y > 0.5f): round(p) == y for 0 / 1 targets
 *     [1] elements         B * O
 *     [2] bad_targets      y outside [0, 1] or not finite; such elements add nothing to the loss, to `correct` or to a gradient
 *     [3] nonfinite_probs
 * lbbnn_elbo_bce_loss_backward: g_probs (B, O dense) = (*g) (p - y) / max((1 - p) p, 1e-12f) (torch's
 *   binary_cross_entropy_backward) and, when g_logits (B, O dense) is given, g_logits = g_probs ((1 - p) p) in the same launch
 *   -- bitwise what lbbnn_sigmoid_backward makes of g_probs; *g_kl = (*g) kl_scale (g_kl nullable).
 * lbbnn_sigmoid_backward: out = g ((1 - p) p), the backward of the head for probabilities that feed another loss. */
int lbbnn_binary_head(const float* logits, int ldi, int B, int O, float* probs, int ldp, float* logp2, int ld2, void* stream);
int lbbnn_elbo_bce_loss(const float* probs, int ldp, const float* target, int ldt, int B, int O, const float* kl, float kl_scale,
                        float* loss, int* stats, int accumulate, void* stream);
int lbbnn_elbo_bce_loss_backward(const float* g, const float* probs, int ldp, const float* target, int ldt, int B, int O,
                                 float kl_scale, float* g_probs, float* g_logits, float* g_kl, void* stream);
int lbbnn_sigmoid_backward(const float* g, int ldg, const float* probs, int ldp, float* out, int ldo, int B, int O, void* stream);
/* lbbnn_elbo_bce_loss_monitor -- lbbnn_elbo_bce_loss with the running totals of a training log and a per-step "loss is not
 * finite" flag, in the SAME single launch of one workgroup: what lbbnn_elbo_loss_monitor is to lbbnn_elbo_loss.  *loss and
 * stats are bitwise what lbbnn_elbo_bce_loss writes for the same arguments (one shared pass: the same terms, added in the same
 * order).  The backward launch is lbbnn_elbo_bce_loss_backward, unchanged.
 * totals / guard: the LBBNN_MONITOR_WORDS int64 words and the int32 word of lbbnn_elbo_loss_monitor, the same layout.  A "row"
 * of this loss is ONE ELEMENT (b, o) of the (B, O) block -- one Bernoulli observation -- so with n = B * O every call adds:
 *   LBBNN_MONITOR_STEPS            1
 *   LBBNN_MONITOR_ROWS             n
 *   LBBNN_MONITOR_CORRECT          elements with a valid target and (p > 0.5f) == (y > 0.5f)              (stats[0])
 *   LBBNN_MONITOR_BAD_TARGETS      elements whose target is outside [0, 1] or NaN: no loss term, no gradient (stats[2])
 *   LBBNN_MONITOR_NONFINITE_ROWS   elements whose p is inf or NaN                                           (stats[3])
 *   LBBNN_MONITOR_NONFINITE_STEPS  1 when *loss is inf or NaN
 *   LBBNN_MONITOR_SKIPPED_STEPS    not written here: the guarded optimizer steps' slot
 *   LBBNN_MONITOR_NLL_ROWS         n - bad_targets, when *loss is finite
 * Sums, with nll = the fp64 sum of the fp32 BCE terms and kl_term = kl ? *kl * kl_scale : 0 in fp64:
 *   LBBNN_MONITOR_NLL_SUM, LBBNN_MONITOR_KL_TERM_SUM, LBBNN_MONITOR_LOSS_SUM   += nll, kl_term, nll + kl_term -- ONLY on a call
 *                                  whose *loss is finite
 *   LBBNN_MONITOR_LAST_NLL, LBBNN_MONITOR_LAST_LOSS   overwritten by every call: nll, and (double)*loss
 * A NaN probability against a valid target is NOT a non-finite loss: max(logf(NaN), -100) is -100 (fmaxf returns its number),
 * so the element costs 100 and is counted in LBBNN_MONITOR_NONFINITE_ROWS; the flag follows *loss alone.
 * guard (nullable): OVERWRITTEN by every call: 1 when *loss is not finite, else 0.  No atomics: thread 0 reads every total
 * ahead of its first store; one monitor may have one such launch in flight at a time (launches of one stream are).
 * Checks (before any HIP call): probs / target / loss / totals NULL: LBBNN_E_NULL; O outside 1..16, B < 1, B * O >= 2^31,
 * ldp < O, ldt < O: LBBNN_E_SHAPE; a pointer off 4 bytes, totals off 8: LBBNN_E_ALIGN.  kl, stats and guard are nullable. */
int lbbnn_elbo_bce_loss_monitor(const float* probs, int ldp, const float* target, int ldt, int B, int O, const float* kl,
                                float kl_scale, float* loss, int* stats, int accumulate, int64_t* totals, int32_t* guard,
                                void* stream);

/* lbbnn_layers_operands_snap + lbbnn_format_x of the network input in the SAME launches: the format job (one pass over x) runs
 * as workgroups behind the rows of the weight-pass launch, whose memory system idles through the rows' compute phase -- no
 * launch of its own.  Falls back to a separate lbbnn_format_x launch when the weight-pass launch cannot carry it (in-kernel
 * flows, rows that take the generic kernel). */
int lbbnn_layers_operands_x(const lbbnn_layer_desc_t* layers, int n, uint64_t* rng, uint64_t* rng_snap, uint64_t advance,
                            const float* x, int ldx, void* planes, int ldp, int B, int I, void* stream);

/* lbbnn_weight_pass producing LBBNN_F_F16S operands + their row scales (single layer; the batched form is
 * lbbnn_layers_operands with split == 2). */
int lbbnn_weight_pass_f16(const float* mu, const float* rho, const float* lambdal,
                          const float* z_fwd, const float* z_kl, const float* r0_c,
                          const float* bias_rho, const lbbnn_priors_t* priors,
                          void* e_w, void* var_w, int ld, float* e_scale, float* v_scale,
                          float* kl_rows, float* act_mu, float* act_var, float* bias_var,
                          int O, int I, int flags /* 0 | LBBNN_F_VAR1 */, void* stream);

/* lbbnn_eval_metrics -- every number the reference's evaluation loops report, from one (S members, B rows, C classes) block of
 * log-probabilities (test_ensemble, LBBNN-GP-MF-MNF.py:312-323; outofsample, :370-392; VD's validation,
 * variational_dropout.py:160-176), with running totals that stay on the device.  No host synchronisation, no allocation.
 * Launches: 1, or 2 with totals (the second, one workgroup, adds the double sums); B == 0: a successful no-op, no launch.
 *
 * Inputs.  logp: member m, row b, class c at logp + m * m_stride + b * ldp + c (64-bit offsets: the padded head buffer of the
 * member GEMMs as it is, or a dense (S,B,C) tensor).  mean_logp (optional): (B,C) rows of stride ldm, the posterior-mean
 * forward.  target (optional): B int64 class indices.  1 <= S <= 65535, B >= 0, 1 <= C <= 64.
 *
 * Per-row outputs, each optional (NULL = not written):
 *   ens_logp[b * C + c]  the mean over the members, with THIS arithmetic: acc = logp[0]; acc += logp[m] for m = 1 .. S-1
 *                        ascending, in fp32; then acc / (float)S by IEEE (correctly rounded) division.  A CPU restatement
 *                        in fp32 reproduces it bit for bit.
 *   pred_ensemble[b]     argmax over c of ens_logp[b] by numpy.argmax's rule: a NaN compares as the maximum, the lowest index
 *                        of the maximum wins (-0 == +0).
 *   pred_mean[b]         the same argmax of mean_logp[b] (needs mean_logp: LBBNN_E_NULL otherwise).
 *   entropy[b]           outofsample's predictive entropy in fp32: per member sigmoid(logp) = 1 / (1 + exp(-logp)) divided by
 *                        its sum over the classes of the row, the mean over the members (sum in member order, / S), then
 *                        -sum_c p log p.  A row where that expression is not finite is stored as computed.
 *
 * Running totals: counts, correct_member, confusion, sums and work are given together or not at all.  They are ADDED TO, so
 * consecutive calls accumulate over batches; the caller zeroes them.
 *   counts[LBBNN_EVAL_COUNTS] (int64), in this order:
 *     rows, rows_with_target (target given and inside [0, C)), bad_targets (target given and outside [0, C); such rows are
 *     left out of every total that needs a target), correct_ensemble (pred_ensemble == target), correct_posterior_mean (the
 *     argmax of mean_logp == target; stays 0 without mean_logp), entropy_nonfinite (rows whose entropy is inf or NaN)
 *   correct_member[S] (int64)   rows whose member-m argmax (same rule) == target: outofsample's `corrects`
 *   confusion[C * C] (int64)    confusion[target * C + pred_ensemble]: rows are the true labels (variational_dropout.py:176)
 *   sums[2] (double)            sums[0] += -sum_b (double)ens_logp[b][target_b]: F.nll_loss(outputs.mean(0), target,
 *                               reduction="sum"), the data term of VD's validation loss;  sums[1] += sum of (double)entropy[b]
 *                               over the rows where it is finite.
 * Every total is bitwise reproducible from run to run: the integer totals are exact (integer atomics), and each workgroup
 * leaves its two double partials in `work`, which the second launch adds in a fixed order -- no float atomics.
 * work: lbbnn_eval_metrics_work_bytes(S, B, C) bytes (> 0 for every valid shape, non-decreasing in B), 8-B aligned.
 *
 * Checks, before anything is launched: a NULL args / logp, some but not all of the totals pointers, totals without work,
 * pred_mean without mean_logp: LBBNN_E_NULL.  S, C or B out of range, ldp < C, ldm < C, and with S > 1 and B > 0 a member stride
 * that does not hold B rows (m_stride < (B - 1) * ldp + C): LBBNN_E_SHAPE.  A pointer off its natural alignment (4 B for the
 * floats, 8 B for int64 / double / work): LBBNN_E_ALIGN. */
#define LBBNN_EVAL_COUNTS 6
typedef struct lbbnn_eval_metrics_args {
    const float* logp;
    int64_t m_stride, ldp;
    const float* mean_logp;
    int64_t ldm;
    const int64_t* target;
    float* ens_logp;
    int64_t* pred_ensemble;
    int64_t* pred_mean;
    float* entropy;
    int64_t* counts;
    int64_t* correct_member;
    int64_t* confusion;
    double* sums;
    void* work;
    int S, B, C;
} lbbnn_eval_metrics_args_t;

int64_t lbbnn_eval_metrics_work_bytes(int S, int B, int C);
int lbbnn_eval_metrics(const lbbnn_eval_metrics_args_t* args, void* stream);

/* lbbnn_eval_uncertainty -- how good the ensemble's uncertainty is, from the same (S members, B rows, C classes) block of
 * log-probabilities lbbnn_eval_metrics reads: the predictive distribution of the Bayesian model average, its entropy split into
 * the expected (aleatoric) part and the mutual information between prediction and parameters (epistemic, BALD), the proper
 * scores (Brier, log score), and running totals for reliability tables (ECE / MCE, accuracy against coverage) and score
 * histograms (AUROC between two passes).  No host synchronisation, no allocation.  Launches: 1, or 2 with totals (the second,
 * one workgroup, adds the double sums); B == 0: a successful no-op, no launch.
 *
 * Inputs.  logp, m_stride, ldp, target, S, B, C: as lbbnn_eval_metrics.  conf_bins M (1..100) and hist_bins K (1..4096) matter
 * with totals only.  ent_scale: the fp32 factor that maps an entropy to a histogram bin, computed by the caller as
 * (float)(K / ln C) and 0 for C == 1 (finite and >= 0, LBBNN_E_SHAPE otherwise); the kernel multiplies by it and never takes
 * log(C) itself, so the bin of a stored value is reproducible on the CPU.
 *
 * Per-row outputs, each optional (NULL = not written), fp32 except the prediction; exp / log are the device's expf / logf:
 *   bma_probs[b * C + c]   pbar: acc = expf(logp[0]); acc += expf(logp[m]) for m = 1 .. S-1 ascending; then acc / (float)S by IEEE
 *                          division.
 *   pred_bma[b] (int64)    argmax over c of bma_probs[b] by numpy.argmax's rule (a NaN is the maximum, the lowest index wins).
 *   confidence[b]          the maximum of bma_probs[b]: the stored value of class pred_bma[b], bit for bit.
 *   total_entropy[b]       -sum_c pbar * logf(pbar), a term being 0 where pbar == 0.  With S == 1, where pbar = expf(l) and its
 *                          logarithm is l itself, the value of expected_entropy[b]: the mutual information of one member is
 *                          then exactly 0.
 *   expected_entropy[b]    h_m = -sum_c expf(l) * l over the classes of member m (a term being 0 where expf(l) == 0), summed
 *                          in member order, / (float)S.
 *   mutual_information[b]  d = total_entropy - expected_entropy; 0 where d < 0 (rounding: the exact value is >= 0), else d -- a
 *                          NaN stays a NaN.
 *   brier[b]               sum_c (pbar_c - [c == target])^2; NaN for a row without a target inside [0, C).
 *   log_score[b]           -(logsumexp_m logp[m][b][target] - logf((float)S)), the log score of pbar at the target, as a
 *                          streaming logsumexp: the running maximum mx of the members seen so far is subtracted before every
 *                          expf (s = s * expf(mx_old - l) + 1 when l raises the maximum, s += expf(l - mx) otherwise; a member
 *                          at -inf adds nothing), then mx + logf(s).  Finite whenever one member's log-probability of the
 *                          target is finite -- -logf(pbar_target) is not (it is inf once every expf underflows).  NaN for a
 *                          row without a valid target.
 *
 * Running totals: counts, sums, the four bin arrays, hist and work are given together or not at all.  They are ADDED TO; the
 * caller zeroes them.  A row is FINITE when its confidence, total entropy, expected entropy and mutual information all are.
 *   counts[LBBNN_UNC_COUNTS] (int64), in this order:
 *     rows, rows_with_target, bad_targets (as lbbnn_eval_metrics), correct_bma (pred_bma == target, every row with a valid
 *     target), nonfinite_rows (rows that are not finite: they enter no sum, bin or histogram below), log_score_nonfinite
 *     (finite rows with a valid target whose log_score is inf or NaN: left out of the log-score sum only)
 *   sums[LBBNN_UNC_SUMS] (double), in this order: total entropy, expected entropy, mutual information, confidence over the
 *     finite rows; Brier over the finite rows with a valid target; log score over those of them where it is finite.
 *   reliability bins, M entries each, bin m = clamp((int)(confidence * (float)M), 0, M - 1):
 *     bin_rows (int64, finite rows), bin_rows_with_target (int64, finite rows with a valid target), bin_correct (int64, those
 *     with pred_bma == target), bin_conf_sum (double, the confidence of the finite rows with a valid target)
 *   hist[3 * K] (int64) over the finite rows, bin k = clamp((int)(v * scale), 0, K - 1): hist[k] of v = total_entropy and
 *     hist[K + k] of v = mutual_information with scale = ent_scale, hist[2 * K + k] of v = 1.0f - confidence with scale =
 *     (float)K.
 *   Every product is a single fp32 multiplication; it is clamped to [0, bins] as a float before the conversion (a product
 *   that overflowed lands in the last bin), so no index is ever taken from a value an int cannot hold.
 * Every total is bitwise reproducible from run to run: the integers are counted per workgroup and added with integer atomics
 * (exact); each workgroup adds its rows' doubles in row order and leaves 6 + M partials in `work`, which the second launch
 * adds in a fixed order -- no float atomics.
 * work: lbbnn_eval_uncertainty_work_bytes(S, B, C, conf_bins) bytes (> 0 for every valid shape, non-decreasing in B; 0 for an
 * invalid one), 8-B aligned.
 *
 * Checks, before anything is launched: a NULL args / logp, some but not all of the totals pointers: LBBNN_E_NULL.  S, C or B
 * out of range, ldp < C, a short m_stride (as lbbnn_eval_metrics), and with totals conf_bins, hist_bins or ent_scale out of
 * range: LBBNN_E_SHAPE.  A pointer off its natural alignment: LBBNN_E_ALIGN. */
#define LBBNN_UNC_COUNTS 6
#define LBBNN_UNC_SUMS 6
typedef struct lbbnn_eval_uncertainty_args {
    const float* logp;
    int64_t m_stride, ldp;
    const int64_t* target;
    float* bma_probs;
    int64_t* pred_bma;
    float* confidence;
    float* total_entropy;
    float* expected_entropy;
    float* mutual_information;
    float* brier;
    float* log_score;
    int64_t* counts;
    double* sums;
    int64_t* bin_rows;
    int64_t* bin_rows_with_target;
    int64_t* bin_correct;
    double* bin_conf_sum;
    int64_t* hist;
    void* work;
    int S, B, C;
    int conf_bins, hist_bins;
    float ent_scale;
} lbbnn_eval_uncertainty_args_t;

int64_t lbbnn_eval_uncertainty_work_bytes(int S, int B, int C, int conf_bins);
int lbbnn_eval_uncertainty(const lbbnn_eval_uncertainty_args_t* args, void* stream);

/* The fused Gaussian ELBO loss of a regression network (head "identity": the last layer's raw output m is the mean of a normal
 * likelihood whose log-variance is lv): F.gaussian_nll_loss(m, y, exp(lv), full=True, reduction='sum') + kl / NUM_BATCHES.  One
 * forward launch of one 1024-thread workgroup, one pass, fp64 partial sums in a fixed order, no atomics: the same bits from run to
 * run.  (B, O) blocks with dense rows and a free row stride (ld*, floats); 0 <= B, 1 <= O <= 16, B * O < 2^31.
 * log_var: ldv == 0: O floats, one noise level per output unit; ldv >= O: a (B, O) block of row stride ldv, one per element.
 *
 * Element (b, o), with y = target, every operation a single fp32 one in this order (no fused multiply-add):
 *   d = y - m;  iv = expf(-lv);  q = (d * d) * iv;  term = 0.5f * ((L + lv) + q);  dlv = 0.5f * (1.f - q)
 *   with L = (float)1.8378770664093453 = log(2 pi).
 * A target that is NaN or infinite is a BAD target: the element has no term, no gradient, and is counted.  A non-finite m or lv
 * makes the term, and with it the loss, non-finite (and is counted, bad target or not).
 * lbbnn_elbo_gaussian_loss:
 *   *loss = (float)(sum_{b,o} (double)term + (kl ? (double)*kl * (double)kl_scale : 0)).  The first T = (1024 / O) * O threads
 *   work, thread t on the elements t, t + T, ... in rising order (all of column t % O); the threads' fp64 sums are added by the
 *   fixed wave butterfly, the 16 wave totals in wave order by one thread after the workgroup's single barrier.
 *   stats (double[4], nullable) is ADDED TO by thread 0 with plain loads and stores (the caller zeroes it):
 *     [0] += sum (double)(d * d)   [1] += sum (double)fabsf(d)   over the elements with a valid target
 *     [2] += elements with a valid target                        [3] += bad targets
 *   lv_cols (O floats, nullable; ldv == 0 only, LBBNN_E_SHAPE otherwise): lv_cols[o] = (float)(sum_b (double)dlv[b][o]) over
 *   the valid targets of column o, the threads of the column added in the same fixed order -- d loss / d lv[o] up to the factor
 *   *g, a by-product of the pass.
 * lbbnn_elbo_gaussian_loss_backward (one multi-workgroup launch): g_mean (B, O dense) = ((*g) * (m - y)) * iv, 0 for a bad
 *   target; g_lv (nullable): ldv >= O: (B, O dense) = ((*g) * 0.5f) * (1.f - (d * d) * iv), 0 for a bad target; ldv == 0: O
 *   floats, g_lv[o] = (*g) * lv_cols[o] with lv_cols as the forward left them (required then: LBBNN_E_NULL);  *g_kl = (*g) *
 *   kl_scale (g_kl nullable).
 * Checks (before any HIP call): a required pointer NULL: LBBNN_E_NULL; B < 0, O outside 1..16, B * O >= 2^31, ldm < O, ldt < O,
 * 0 < ldv < O or ldv < 0, lv_cols with ldv != 0: LBBNN_E_SHAPE; a pointer off 4 bytes, stats off 8: LBBNN_E_ALIGN. */
int lbbnn_elbo_gaussian_loss(const float* mean, int ldm, const float* target, int ldt, const float* log_var, int ldv, int B, int O,
                             const float* kl, float kl_scale, float* loss, double* stats, float* lv_cols, void* stream);
int lbbnn_elbo_gaussian_loss_backward(const float* g, const float* mean, int ldm, const float* target, int ldt,
                                      const float* log_var, int ldv, int B, int O, float kl_scale, const float* lv_cols,
                                      float* g_mean, float* g_lv, float* g_kl, void* stream);
/* lbbnn_elbo_gaussian_loss_monitor -- lbbnn_elbo_gaussian_loss with the running totals of a training log and a per-step "loss is
 * not finite" flag, in the SAME single launch of one workgroup.  *loss, stats and lv_cols are bitwise what
 * lbbnn_elbo_gaussian_loss writes for the same arguments (one shared pass).  The backward launch is unchanged.
 * totals / guard: the LBBNN_MONITOR_WORDS int64 words and the int32 word of lbbnn_elbo_loss_monitor, the same layout.  A "row" is
 * ONE ELEMENT (b, o), as for lbbnn_elbo_bce_loss_monitor; with n = B * O every call adds:
 *   LBBNN_MONITOR_STEPS            1
 *   LBBNN_MONITOR_ROWS             n
 *   LBBNN_MONITOR_CORRECT          elements with a valid target and fabsf(d) <= expf(0.5f * lv): inside one standard deviation
 *                                  (the share of them is the one-sigma coverage, 0.683 for a calibrated normal)
 *   LBBNN_MONITOR_BAD_TARGETS      elements whose target is NaN or infinite                                  (stats[3])
 *   LBBNN_MONITOR_NONFINITE_ROWS   elements whose m or lv is inf or NaN
 *   LBBNN_MONITOR_NONFINITE_STEPS  1 when *loss is inf or NaN
 *   LBBNN_MONITOR_SKIPPED_STEPS    not written here: the guarded optimizer steps' slot
 *   LBBNN_MONITOR_NLL_ROWS         n - bad_targets, when *loss is finite
 * Sums, with nll = the fp64 sum of the fp32 terms and kl_term = kl ? *kl * kl_scale : 0 in fp64: as
 * lbbnn_elbo_bce_loss_monitor (NLL_SUM, KL_TERM_SUM, LOSS_SUM only on a call whose *loss is finite; LAST_NLL, LAST_LOSS
 * overwritten by every call).  guard (nullable): OVERWRITTEN by every call: 1 when *loss is not finite, else 0.
 * Checks: those of lbbnn_elbo_gaussian_loss with B < 1: LBBNN_E_SHAPE, and totals NULL: LBBNN_E_NULL; totals off 8 bytes, guard
 * off 4: LBBNN_E_ALIGN. */
int lbbnn_elbo_gaussian_loss_monitor(const float* mean, int ldm, const float* target, int ldt, const float* log_var, int ldv,
                                     int B, int O, const float* kl, float kl_scale, float* loss, double* stats, float* lv_cols,
                                     int64_t* totals, int32_t* guard, void* stream);

/* lbbnn_eval_regression -- the evaluation numbers of a regression ensemble, from one (S members, B rows, O units) block of raw
 * outputs (the member GEMMs of an identity-head network) under a normal likelihood with log-variance lv = log_var[o] per output
 * unit, with running totals that stay on the device.  No host synchronisation, no allocation.  Launches: 1, or 2 with totals
 * (the second, one workgroup, adds the double sums); B == 0: a successful no-op, no launch.
 *
 * Inputs.  out: member s, row b, unit o at out + s * m_stride + b * ldp + o (64-bit offsets: the padded buffer of the member
 * GEMMs as it is, or a dense (S, B, O) tensor).  mean_out (optional): (B, O) rows of stride ldm, the posterior-mean forward.
 * target (optional): (B, O) fp32 rows of stride ldt; a NaN or infinite target is a BAD target.  log_var: O floats, read through
 * the pointer by every call (a live parameter).  1 <= S <= 65535, B >= 0, 1 <= O <= 16, B * O < 2^31.
 *
 * Per-element outputs (B * O dense, element b * O + o), each optional (NULL = not written).  m_s is member s's output, y the
 * target; every operation is a single fp32 one in the order written (no fused multiply-add); expf / logf / erfcf / sqrtf are the
 * device's:
 *   pred_mean      acc = m_0; acc += m_s for s = 1 .. S-1 ascending; then acc / (float)S by IEEE division.  A CPU restatement in
 *                  fp32 reproduces it bit for bit.
 *   epistemic_var  d_s = m_s - pred_mean; acc = d_0 * d_0; acc += d_s * d_s ascending; then acc / (float)S.  Bit-reproducible too.
 *   aleatoric_var  expf(lv)
 *   total_std      sqrtf(epistemic_var + aleatoric_var)
 *   sq_err         e = y - pred_mean; e * e.  NaN without a valid target.
 *   log_density    the log of the members' mixture density at y: with r_s = y - m_s, iv = expf(-lv), L = (float)log(2 pi) and
 *                  t_s = -0.5f * ((L + lv) + (r_s * r_s) * iv), the streaming logsumexp of lbbnn_eval_uncertainty's log_score
 *                  (s = s * expf(mx_old - t) + 1 when t raises the running maximum mx, s += expf(t - mx) otherwise; a term at -inf
 *                  adds nothing), then (mx + logf(s)) - logf((float)S).  Finite whenever one member's term is finite, where
 *                  logf(mean expf(t_s)) is -inf once every expf underflows.  NaN without a valid target.
 *   pit            the probability integral transform of y under the mixture: with hs = expf(-0.5f * lv),
 *                  Phi_s = 0.5f * erfcf(-((r_s * hs) * (float)(1 / sqrt 2))); acc = Phi_0; acc += Phi_s ascending; acc / (float)S.
 *                  NaN without a valid target.
 *
 * Running totals: counts, sums, pit_hist and work are given together or not at all.  They are ADDED TO; the caller zeroes them.
 * An element is FINITE when lv and every member's output are; it is SCORED when it is finite and has a valid target.
 *   counts[LBBNN_REG_COUNTS] (int64), in this order: elements, elements with a valid target, bad targets (target given and NaN
 *     or infinite), non-finite elements (they enter no sum and no bin), scored elements
 *   sums[LBBNN_REG_SUMS] (double), in this order: sq_err, |y - pred_mean|, log_density, y, y * y (fp32 product) and the squared
 *     error (y - mean_out)^2 of the posterior-mean forward (0 without mean_out) over the SCORED elements -- at positions 0, 1, 2,
 *     5, 6, 7 -- and epistemic_var, epistemic_var + aleatoric_var over the FINITE elements at positions 3, 4
 *   pit_hist[pit_bins] (int64) over the scored elements, bin = clamp((int)(pit * (float)pit_bins), 0, pit_bins - 1): a single fp32
 *     product, clamped to [0, pit_bins] as a float before the conversion.  1 <= pit_bins <= 1024.
 * Every total is bitwise reproducible from run to run: the integers are counted per workgroup and added with integer atomics
 * (exact); each workgroup of 256 consecutive elements adds its doubles in element order and leaves LBBNN_REG_SUMS partials in
 * `work`, which the second launch adds in a fixed order -- no float atomics.
 * work: lbbnn_eval_regression_work_bytes(S, B, O) bytes (> 0 for every valid shape, non-decreasing in B; 0 for an invalid one),
 * 8-B aligned.
 *
 * Checks, before anything is launched, in this order: a NULL args / out / log_var, some but not all of the totals pointers:
 * LBBNN_E_NULL.  S, O or B out of range, ldp < O, ldm < O with mean_out, ldt < O with target, a short m_stride (S > 1, B > 0,
 * m_stride < (B - 1) * ldp + O), B * O >= 2^31, and with totals pit_bins out of range: LBBNN_E_SHAPE.  A pointer off its natural
 * alignment (4 B for the floats, 8 B for int64 / double / work): LBBNN_E_ALIGN. */
#define LBBNN_REG_COUNTS 5
#define LBBNN_REG_SUMS 8
typedef struct lbbnn_eval_regression_args {
    const float* out;
    int64_t m_stride, ldp;
    const float* mean_out;
    int64_t ldm;
    const float* target;
    int64_t ldt;
    const float* log_var;
    float* pred_mean;
    float* epistemic_var;
    float* aleatoric_var;
    float* total_std;
    float* sq_err;
    float* log_density;
    float* pit;
    int64_t* counts;
    double* sums;
    int64_t* pit_hist;
    void* work;
    int S, B, O;
    int pit_bins;
} lbbnn_eval_regression_args_t;

int64_t lbbnn_eval_regression_work_bytes(int S, int B, int O);
int lbbnn_eval_regression(const lbbnn_eval_regression_args_t* args, void* stream);

/* lbbnn_eval_regression_scores -- lbbnn_eval_regression for a heteroscedastic ensemble, with two more scores: the numbers above
 * from one (S members, B rows, O units) block of member means under a normal likelihood whose log-variance operand has strides of
 * its own, plus the CRPS of the members' mixture and central prediction intervals, with running totals that stay on the device.
 * No host synchronisation, no allocation.  Launches: 1, or 2 with totals; B == 0: a successful no-op, no launch.
 *
 * Inputs.  out, m_stride, ldp, mean_out, ldm, target, ldt: as lbbnn_eval_regression (of mean_out only columns [0, O) are read).
 * log_var: member s, row b, unit o at log_var + s * lv_mstride + b * lv_ld + o, read through the pointer by every call:
 *   (lv_mstride, lv_ld) = (0, 0)    one value per unit, log_var[o]
 *                         (0, ld)   one value per element, shared by the members; ld >= O
 *                         (ms, ld)  one value per member and element; ld >= O, ms >= (B - 1) * ld + O when S > 1 and B > 0
 * The last form may point INTO the buffer of `out` at a column offset: a (S, B, 2 O) ensemble output with means in columns [0, O)
 * and log-variances in [O, 2 O) is out = buf, log_var = buf + O, lv_mstride = m_stride, lv_ld = ldp, read in place.
 * levels[n_levels]: central interval levels p, 0 <= n_levels <= LBBNN_SCORE_MAX_LEVELS, each in [0.01, 0.999] (host values).
 * 1 <= S <= LBBNN_SCORE_MAX_MEMBERS (the CRPS is quadratic in S), B >= 0, 1 <= O <= 16, B * O < 2^31.
 *
 * An element is FINITE when every member's mean is finite and every member's log-variance has |lv_s| <= 80 (a NaN fails; the
 * bound keeps expf(+-lv) normal in fp32); it is SCORED when it is finite and has a valid target.  A non-finite element gets NaN
 * in EVERY per-element output and enters no sum and no bin.
 *
 * Per-element outputs, each optional, (B, O) dense, element e = b * O + o; lower / upper / interval_score are (n_levels, B, O),
 * level l at l * B * O + e.  m_s, lv_s: member s's mean and log-variance, y the target; single fp32 operations in the order
 * written unless stated (no fused multiply-add); expf / logf / erfcf / erff / sqrtf are the device's:
 *   pred_mean, epistemic_var   lbbnn_eval_regression's expressions and order: the same bits for a finite element
 *   aleatoric_var  acc = expf(lv_0); acc += expf(lv_s) ascending; acc / (float)S
 *   total_std      sqrtf(epistemic_var + aleatoric_var)
 *   sq_err, log_density, pit   lbbnn_eval_regression's with lv_s for lv: t_s = -0.5f * ((L + lv_s) + (r_s * r_s) * expf(-lv_s)) in
 *                  the streaming logsumexp; Phi_s = 0.5f * erfcf(-((r_s * expf(-0.5f * lv_s)) * (float)(1 / sqrt 2))).  NaN
 *                  without a valid target.
 *   crps           the continuous ranked probability score of the mixture at y in closed form (Grimit et al. 2006).  With
 *                  A(m, v) = 2 sd phi(z) + |m| erff(z / sqrt 2), sd = sqrtf(v), z = |m| / sd (= E|N(m, v)|, both terms >= 0) and
 *                  v_s = expf(lv_s):  crps = (1 / S) sum_s A(y - m_s, v_s) - (1 / 2 S^2) sum_{s,t} A(m_s - m_t, v_s + v_t).
 *                  Each A is fp32; both sums are accumulated in DOUBLE -- the first over s ascending, the second as
 *                  sum_s [A(0, 2 v_s) + 2 sum_{t < s} A(m_s - m_t, v_s + v_t)], s and t ascending -- combined in double and
 *                  rounded to fp32 once.  NaN without a valid target.
 *   lower, upper   the (1 - p) / 2 and (1 + p) / 2 quantiles of the mixture CDF F(x) = pit's expression at x: 26 bisection steps
 *                  from the bracket [min_s (m_s - 8 sd_s), max_s (m_s + 8 sd_s)] (F(mid) < target raises the lower end), the
 *                  midpoint of the last bracket returned.  A fixed iteration count: deterministic, and lower <= upper always.
 *   interval_score (u - l) + (2.f / (1.f - p)) * (fmaxf(l - y, 0) + fmaxf(y - u, 0)).  NaN without a valid target.
 *
 * Running totals: counts, sums, pit_hist and work are given together or not at all.  They are ADDED TO; the caller zeroes them.
 *   counts[LBBNN_SCORE_COUNTS] (int64): the five of lbbnn_eval_regression, then inside[l], l < LBBNN_SCORE_MAX_LEVELS: the scored
 *     elements with lower_l <= y <= upper_l (levels >= n_levels are not touched)
 *   sums[LBBNN_SCORE_SUMS] (double): the eight of lbbnn_eval_regression at the same positions (total variance = epistemic_var +
 *     aleatoric_var), then aleatoric_var over the FINITE elements at 8, crps over the SCORED elements at 9, width_l = upper_l -
 *     lower_l over the scored elements at 10 + l and interval_score_l at 10 + LBBNN_SCORE_MAX_LEVELS + l
 *   pit_hist[pit_bins] (int64): as lbbnn_eval_regression.
 * Every total is bitwise reproducible from run to run, by the construction of lbbnn_eval_regression's: integer atomics for the
 * integers; each workgroup -- 64 consecutive elements here -- adds its doubles in element order and leaves LBBNN_SCORE_SUMS
 * partials in `work`, which the second launch adds in a fixed order.
 * work: lbbnn_eval_regression_scores_work_bytes(S, B, O, n_levels) bytes (> 0 for every valid shape, non-decreasing in B; 0 for
 * an invalid one), 8-B aligned.
 *
 * Checks, before anything is launched, in this order: a NULL args / out / log_var, some but not all of the totals pointers:
 * LBBNN_E_NULL.  S, O or B out of range, ldp < O, ldm < O with mean_out, ldt < O with target, a short m_stride, B * O >= 2^31,
 * 0 < lv_ld < O, lv_mstride < 0, lv_mstride != 0 with lv_ld == 0, a short lv_mstride (S > 1, B > 0, 0 < lv_mstride <
 * (B - 1) * lv_ld + O), n_levels out of range, a level outside [0.01, 0.999] (or NaN), and with totals pit_bins out of range:
 * LBBNN_E_SHAPE.  A pointer off its natural alignment: LBBNN_E_ALIGN. */
#define LBBNN_SCORE_MAX_LEVELS 4
#define LBBNN_SCORE_MAX_MEMBERS 64
#define LBBNN_SCORE_COUNTS (LBBNN_REG_COUNTS + LBBNN_SCORE_MAX_LEVELS)
#define LBBNN_SCORE_SUMS (LBBNN_REG_SUMS + 2 + 2 * LBBNN_SCORE_MAX_LEVELS)
typedef struct lbbnn_eval_scores_args {
    const float* out;
    int64_t m_stride, ldp;
    const float* mean_out;
    int64_t ldm;
    const float* target;
    int64_t ldt;
    const float* log_var;
    int64_t lv_mstride, lv_ld;
    float* pred_mean;
    float* epistemic_var;
    float* aleatoric_var;
    float* total_std;
    float* sq_err;
    float* log_density;
    float* pit;
    float* crps;
    float* lower;
    float* upper;
    float* interval_score;
    int64_t* counts;
    double* sums;
    int64_t* pit_hist;
    void* work;
    int S, B, O;
    int pit_bins;
    int n_levels;
    float levels[LBBNN_SCORE_MAX_LEVELS];
} lbbnn_eval_scores_args_t;

int64_t lbbnn_eval_regression_scores_work_bytes(int S, int B, int O, int levels);
int lbbnn_eval_regression_scores(const lbbnn_eval_scores_args_t* args, void* stream);

/* ------------------------------------------------------------------------------------------------------------------------------
 * lbbnn_gate_structure: the posterior over the STRUCTURES of a latent-binary network -- per sample the hard gates of every layer
 * are drawn and the units some output depends on are found (evaluate.live_structure's sweep), in ONE launch for the whole
 * network and all samples, without storing a gate.  Integers only: every output is exact and the same bits on every run.
 *
 * layers[l], l < n: lambdal (O, I) with rows ld floats apart, and the layer's Philox id.  Boundary b of the network, b = 0 .. n:
 * 0 = the input features (width layers[0].I), b = the outputs of layer b - 1 (width layers[b - 1].O).  For sample s < samples:
 *   gamma_l[o][i] = u < alpha, alpha = 1 / (1 + expf(-lambdal[o][i])) in fp32 (the device's expf), u = ((bits >> 8) + 0.5) 2^-24
 *     from word i % 4 of Philox counter (o, i / 4) of stream LBBNN_STREAM_GATE * 64 + layer_id at state {rng[0], rng[1] + s}: the
 *     hard draw of lbbnn_gate_sample_draw / lbbnn_gate_members (exact bit 8), bit for bit.  A NaN lambdal is never kept.
 *   need[n][o] = 1;  need[l][i] = any_o(need[l + 1][o] & gamma_l[o][i])
 *   kept[s * n + l]         = sum_{o,i} gamma_l[o][i]                    (every weight is drawn, needed row or not)
 *   needed[s * (n + 1) + b] = sum_j need[b][j]
 *   active[s * n + l]       = sum_{o : need[l + 1][o]} sum_i gamma_l[o][i]   (such a weight's column is needed by construction)
 *   need_out (nullable): [samples][width] uint8 in {0, 1}, width = lbbnn_gate_structure_width(layers, n) = the widths of all
 *     n + 1 boundaries; boundary b of sample s starts at s * width + (the widths of boundaries 0 .. b - 1).
 * Totals over the samples, ADDED TO (integer atomics; the caller zeroes them, so chunks of samples accumulate):
 *   feature_count[i] += sum_s need[0][i];  unit_count (nullable): the hidden boundaries 1 .. n - 1 one after the other,
 *   unit_count[(widths of boundaries 1 .. b - 1) + j] += sum_s need[b][j].
 * The caller advances rng afterwards (by `samples`).  Nothing is read back or allocated: the call can be captured in a graph.
 *
 * Checks, before anything is launched, in this order: layers / kept / needed / active / feature_count NULL: LBBNN_E_NULL; n
 * outside 1 .. LBBNN_STRUCTURE_MAX_LAYERS, samples outside 1 .. 65535: LBBNN_E_SHAPE; per layer a NULL lambdal: LBBNN_E_NULL, O
 * or I outside 1 .. LBBNN_STRUCTURE_MAX_WIDTH, ld < I, I != the O of the layer below: LBBNN_E_SHAPE, lambdal off a 4-B
 * boundary: LBBNN_E_ALIGN; an output off a 4-B boundary: LBBNN_E_ALIGN; rng NULL: LBBNN_E_NOISE.  lambdal rows are read as
 * float4 when I % 4 == 0, ld % 4 == 0 and the base is 16-B aligned, element by element otherwise.
 * lbbnn_gate_structure_width: the width above, or 0 for layers the call would refuse. */
#define LBBNN_STRUCTURE_MAX_LAYERS 16
#define LBBNN_STRUCTURE_MAX_WIDTH 4096
typedef struct lbbnn_structure_desc {
    const float* lambdal;
    int O, I, ld;
    uint32_t layer_id;
} lbbnn_structure_desc_t;

int64_t lbbnn_gate_structure_width(const lbbnn_structure_desc_t* layers, int n);
int lbbnn_gate_structure(const lbbnn_structure_desc_t* layers, int n, int samples, const uint64_t* rng,
                         int32_t* kept, int32_t* needed, int32_t* active, int32_t* feature_count, int32_t* unit_count,
                         uint8_t* need_out, void* stream);

/* ------------------------------------------------------------------------------------------------------------------------------
 * Local explanations of a frozen posterior-mean forward (evaluate.explain).  That forward is a ReLU chain on fixed operands
 * W_1 .. W_L, b_1 .. b_L, so for every row b its pre-head output is EXACTLY linear in the input:
 *   logits[b, c] = sum_i J[b, c, i] x[b, i] + k[b, c],   J(b) = W_L D_{L-1}(b) W_{L-1} .. D_1(b) W_1,   D_l(b) = diag(h_l[b] > 0)
 * The sweep keeps G_l = rows t(b, c) of W_L D_{L-1} .. W_{l+1} D_l as a (B * C', width of h_l) fp32 matrix, row b * C' + c.  Its
 * matrix products G_l W_l are lbbnn_lrt_gemm calls (LBBNN_F_MEAN_ONLY) on transposed fp32 operands; lbbnn_explain_step is
 * everything between two of them.  C' <= LBBNN_EXPLAIN_MAX_OUTPUTS rows of G share an input row; t(b, c) = c without targets,
 * targets[b] (C' == 1; values outside [0, w_rows) are clamped: the caller checks them) with.
 *
 * lbbnn_explain_step, by mode (h: the (B, width) activations of the forward that produced the logits, rows ldh apart):
 *   LBBNN_EXPLAIN_SEED    g[r][j] = w[t][j] * [h[b][j] > 0];  intercept[r] = bias_out[t] + <g[r], bias>;  active[b * ld_active] =
 *                         #{j : h[b][j] > 0};  mask_out (nullable): [h[b][j] > 0] as bytes, rows ldm apart.  w: the LAST layer's
 *                         operand as fp32 rows [w_rows][ldw], so that layer needs no product.
 *   LBBNN_EXPLAIN_MASK    g[r][j] *= [h[b][j] > 0] in place;  intercept[r] += <g[r], bias>;  active and mask_out as above.
 *   LBBNN_EXPLAIN_FINISH  h = the input rows x.  contributions[r][map[i]] = g[r][i] * x[b][i] (map NULL: the identity, and
 *                         full_width == width; with a map the caller zeroes contributions: columns no map entry names are not
 *                         written);  residual[r] = logits[b * ldl + t] - (sum_i g[r][i] x[b][i] + intercept[r]), the sum taken over
 *                         the stored fp32 products.  g == NULL (a network of ONE layer): g[r] = w[t] and intercept[r] = bias_out[t]
 *                         is written here.
 * One wave per input row; every dot product and row sum is a per-lane sum in column order followed by a fixed-order wave
 * reduction: the same bits on every run.  Nothing is read back or allocated.
 *
 * Checks, before anything is launched, in this order: args, h, intercept, the pointers the mode needs (seed / mask: g, bias,
 * active; finish: logits, contributions, residual; seed and a finish without g: w, bias_out) NULL: LBBNN_E_NULL.  An unknown
 * mode, B < 0, width < 1, C outside 1 .. LBBNN_EXPLAIN_MAX_OUTPUTS, B * C > LBBNN_EXPLAIN_MAX_ROWS, a row stride below its
 * width (ldh, ldg, ldw, ldm; ldl < w_rows; ldc < full_width), targets with C != 1, C > w_rows without targets, w_rows < 1 where
 * w or logits are read, ld_active < 1, full_width < width (with map) or != width (without): LBBNN_E_SHAPE.  A pointer off its
 * natural alignment: LBBNN_E_ALIGN.  B == 0: nothing to do, 0.  Rows are read as float4 where the width, the strides and the
 * bases allow it, element by element otherwise.
 *
 * lbbnn_explain_totals: running totals of a batch of contributions (B * C' rows of I columns, rows ldc apart) by output:
 *   sum[cls][i] += sum_r contributions[r][i],  abs_sum[cls][i] += sum_r |contributions[r][i]|,  rows[cls] += #r   over the rows r
 *   of output cls -- r = b * C + cls without targets (C' == C), r = b with targets[b] == cls (C' == 1; clamped into [0, C)).
 * sum / abs_sum: (C, I) doubles, rows: (C) int64, ADDED TO.  Two launches: per-workgroup fp64 column partials into `work`
 * (lbbnn_explain_work_bytes(B, C, I) bytes, 8-B aligned; 0 for a shape the call refuses), rows in order, then one workgroup adds
 * the partials block by block.  The order of every addition depends on the shapes alone: no float atomics, the same bits on
 * every run.  Checks: a NULL pointer (targets may be): LBBNN_E_NULL; B < 0, C outside 1 .. LBBNN_EXPLAIN_MAX_OUTPUTS, I < 1,
 * ldc < I, more than LBBNN_EXPLAIN_MAX_ROWS rows: LBBNN_E_SHAPE; alignment: LBBNN_E_ALIGN; B == 0: 0.
 *
 * lbbnn_explain_operand: out[o][k] = hi + lo (exact in fp32) of an LBBNN_F_SPLIT16 operand [O][ld], as fp32 rows [O][ld]: the
 * value the forward's products multiply by.  NULL: LBBNN_E_NULL; O, I < 1, ld < I: LBBNN_E_SHAPE; ld % 32 or a base off 16 B:
 * LBBNN_E_ALIGN. */
#define LBBNN_EXPLAIN_SEED 0
#define LBBNN_EXPLAIN_MASK 1
#define LBBNN_EXPLAIN_FINISH 2
#define LBBNN_EXPLAIN_MAX_OUTPUTS 16
#define LBBNN_EXPLAIN_MAX_ROWS (1 << 24)
typedef struct lbbnn_explain_step_args {
    int mode;
    int B, C, width;
    float* g;
    int64_t ldg;
    const float* w;
    int64_t ldw;
    int w_rows;
    const int64_t* targets;
    const float* h;
    int64_t ldh;
    const float* bias;
    const float* bias_out;
    float* intercept;
    int32_t* active;
    int64_t ld_active;
    uint8_t* mask_out;
    int64_t ldm;
    const float* logits;
    int64_t ldl;
    const int32_t* map;
    int full_width;
    float* contributions;
    int64_t ldc;
    float* residual;
} lbbnn_explain_step_args_t;

int lbbnn_explain_step(const lbbnn_explain_step_args_t* args, void* stream);
int64_t lbbnn_explain_work_bytes(int B, int C, int I);
int lbbnn_explain_totals(const float* contributions, int64_t ldc, const int64_t* targets, int B, int C, int I,
                         double* sum, double* abs_sum, int64_t* rows, void* work, void* stream);
int lbbnn_explain_operand(const void* op, int O, int I, int ld, float* out, void* stream);

/* ------------------------------------------------------------------------------------------------------------------------------
 * Explanations of sampled-weight members of the sparse median-probability model (evaluate.explain_ensemble).  A member draws
 * explicit weights on the kept pattern -- w[m][k] = mean[k] * z_m[col[k]] + sqrt(var[k]) * eps, b[m][o] = bias_mu[o] +
 * sqrt(bias_var[o]) * eps -- and is then an ordinary ReLU network, so its pre-head output is exactly linear in the input and
 * J_m(b) * x is well defined (the local-reparameterisation member of lbbnn_sparse_layer_members draws per activation and is
 * not).  All buffers between the launches are TRANSPOSED, [block][unit][ld] with the batch row fastest, as in
 * lbbnn_sparse_layer_members.  Every store is a plain vector store; no atomics; sums are sequential or added in a fixed order.
 *
 * lbbnn_sparse_draw_members: ONE launch for all n <= LBBNN_MAX_LAYERS layers and all members.  One thread draws four
 *   consecutive CSR slots (or four units' biases) from one philox_normal4 call at {rng[0], rng[1] + m}:
 *     w[m * w_mstride + k] = fmaf(v_sqrt_f32(var[k]), eps, mean[k] * z[m * z_mstride + col[k]])    stream LBBNN_STREAM_EPS_W * 64 +
 *                            layer_id, counter (k / 4, 0), word k % 4;  z == NULL: no z factor
 *     b[m * b_mstride + o] = fmaf(v_sqrt_f32(bias_var[o]), eps, bias_mu[o])                          stream LBBNN_STREAM_EPS_B * 64 +
 *                            layer_id, counter (o / 4, 0), word o % 4
 *   With tpos / wt (both or neither, else LBBNN_E_NULL) the same value is also stored at wt[m * w_mstride + tpos[k]] (tpos
 *   clamped into [0, nnz)): with tpos the inverse of tslot, wt holds the member's values column by column, the order in which
 *   the sweep walks them.
 *   LBBNN_F_MEAN_ONLY: eps = 0 and nothing is drawn (rng may be NULL).  A member's w / b block is written in whole 16-B quads:
 *   w_mstride >= pad4(nnz), b_mstride >= pad4(O), the tail of the last quad is 0.  col is clamped into [0, I).
 *   NULL layers, bias_mu / bias_var / b, or col / mean / var / w with nnz > 0: LBBNN_E_NULL; n outside [1, LBBNN_MAX_LAYERS],
 *   members outside [1, 65535], O < 1, I < 1, nnz < 0, a member stride below its padded row, z_mstride < I: LBBNN_E_SHAPE; flags
 *   other than 0 | LBBNN_F_MEAN_ONLY: LBBNN_E_FLAGS; rng == NULL without LBBNN_F_MEAN_ONLY: LBBNN_E_NOISE; w / b off a 16-B
 *   boundary or a stride of theirs not a multiple of 4, any other pointer off 4 B (rng: 8 B): LBBNN_E_ALIGN.
 *
 * lbbnn_sparse_gather_members: the member layer on stored values, for `blocks` grid blocks (gridDim.z) of which every
 *   `per_member` consecutive ones belong to one member (m = block / per_member).  With ptr (N + 1) / idx (nnz) a CSR-shaped
 *   pattern over N output units whose entries name input lines in [0, K) (clamped), k running over ptr[u] .. ptr[u + 1] - 1:
 *     s[u][b] = sum_k w[m * w_mstride + (slot ? slot[k] : k)] * a[ablock * a_mstride + idx[k] * lda + b]
 *   sequential fp32 FMAs from 0 in pattern order.  ablock = block, or block % per_member with a_shared (the one-hot seed every
 *   member shares).  Then, by mode:
 *     LBBNN_GATHER_FORWARD  out = s + bias[m * b_mstride + u], then ReLU with `relu`                    (pattern: row_ptr / col)
 *     LBBNN_GATHER_SWEEP    out = h[m * h_mstride + u * ldh + b] > 0 ? s : 0                            (pattern: col_ptr / trow,
 *                           G_l = D_l W_{l+1}^T G_{l+1}; values column by column -- wt of the draw -- or w with slot = tslot)
 *     LBBNN_GATHER_FINISH   out = s * h[u * ldh + b]   with h = x^T, shared by all blocks: the contributions J * x, transposed
 *   out[block * o_mstride + u * ldo + b] (out_rows == 0) or out[block * o_mstride + b * ldo + u] (out_rows != 0).
 *   With dot_bias / dot_acc (both or neither, else LBBNN_E_NULL; not with a_shared: LBBNN_E_FLAGS) extra workgroups of the same
 *   launch add the bias path of the layer whose G is the input: dot_acc[(m * B + b) * per_member + c] += sum_u a[block * a_mstride
 *   + u * lda + b] * dot_bias[m * dot_b_mstride + u] -- four sequential FMA chains over the quarters ceil(K / 4) of u = 0 .. K - 1,
 *   added in order (block = m * per_member + c).  This is how the intercept gathers its hidden layers' terms without a launch.
 *   One lane per batch row (two when B > 64 and the strides allow 8-B words), four units per wave; pattern and values are
 *   wave-uniform scalar loads.  The bits of a number depend on its block, row and unit alone.
 *   B == 0: 0.  args, ptr, w / idx with nnz > 0, a, out, bias (forward) or h (sweep, finish) NULL (slot is nullable):
 *   LBBNN_E_NULL; B < 0 or more than 65535 * 64 rows, K, N < 1, nnz < 0, blocks outside
 *   [1, 65535], per_member < 1 or not dividing blocks, lda / ldh < B, ldo below the layout's need, a negative stride, an
 *   output block stride that does not hold a block, an input block of 2 GiB or more: LBBNN_E_SHAPE; an unknown mode:
 *   LBBNN_E_FLAGS; a pointer off 4 B: LBBNN_E_ALIGN.
 *
 * lbbnn_explain_seed: where the sweep starts, one lane per line position b < ld.  t(b, c') = c' (no targets, Cp == C), targets[b]
 *   (Cp == 1, clamped into [0, C)) or, with pred (Cp == 1), the first largest of mean_m logits[(m * B + b) * C + c] (fp32 sum in
 *   member order, / S), which is also written to targets_out[b].  seed[(c' * C + c) * ld + b] = (b < B && c == t) -- the one-hot
 *   G_L shared by the members -- and intercept[(m * B + b) * Cp + c'] = bias[m * b_mstride + t], the last layer's bias.
 *   rng_live (nullable): rng_live[1] += advance by one lane -- the live Philox offset moves on behind the launches that drew.
 *   B == 0: 0.  bias / seed / intercept, or logits / targets_out with pred NULL: LBBNN_E_NULL; S outside [1, 65535], B < 0, C < 1,
 *   ld < B, Cp != 1 with targets or pred, Cp != C without, b_mstride < C with S > 1: LBBNN_E_SHAPE; pred with targets:
 *   LBBNN_E_FLAGS; alignment (rng_live: 8 B): LBBNN_E_ALIGN.
 *
 * lbbnn_explain_member_stats: statistics over the S members of contributions t[(m * C + c) * t_mstride + i * ldt + b] (what
 *   LBBNN_GATHER_FINISH wrote), as row-major (B, C, F) tensors: mean = (sum_m v) / S with the sum in fp64 in member order; std
 *   = sqrt(sum_m (v - mean)^2 / (S - 1)) in fp64, as (sum d^2 - (sum d)^2 / S) with d = v - v_0 shifted by the first member (one pass; 0 for S == 1); prob_pos / prob_neg = #{m : v > 0} / S and
 *   #{m : v < 0} / S from integer counts; members (nullable) [m][b][c][i] = v.  A 64 x 64 (feature x row) tile goes through
 *   LDS so that both the loads and the stores are coalesced.  With residual (nullable; needs logits and intercept):
 *   residual[(m * B + b) * C + c] = logits[(m * B + b) * ldl + t] - (sum_i v + intercept[(m * B + b) * C + c]) in fp64 with the
 *   sum over i in index order; t = c without targets, targets[b] (C == 1, clamped into [0, n_logits)) with.
 *   B == 0: 0.  args / t / mean / std / prob_pos / prob_neg NULL, residual without logits / intercept: LBBNN_E_NULL; S outside
 *   [1, 65535], C < 1, S * C > 65535, F < 1, B < 0, ldt < B, t_mstride < (F - 1) * ldt + B, targets with C != 1, ldl < n_logits,
 *   C > n_logits without targets: LBBNN_E_SHAPE; a pointer off its natural alignment: LBBNN_E_ALIGN. */
#define LBBNN_GATHER_FORWARD 0
#define LBBNN_GATHER_SWEEP 1
#define LBBNN_GATHER_FINISH 2
typedef struct lbbnn_sparse_draw_desc {
    const int32_t* col;                              /* (nnz)                                   */
    const float *mean, *var;                         /* (nnz)                                   */
    const float *bias_mu, *bias_var;                 /* (O)                                     */
    const float* z;                                  /* [members][z_mstride] or NULL            */
    int64_t z_mstride;
    const int32_t* tpos;                             /* (nnz) or NULL: place of slot k in wt    */
    float* wt;                                       /* [members][w_mstride] or NULL, with tpos */
    float* w;                                        /* [members][w_mstride]                    */
    int64_t w_mstride;
    float* b;                                        /* [members][b_mstride]                    */
    int64_t b_mstride;
    int O, I, nnz;
    uint32_t layer_id;
} lbbnn_sparse_draw_desc_t;

typedef struct lbbnn_sparse_gather_args {
    const int32_t *ptr, *idx, *slot;
    const float* w;
    int64_t w_mstride;
    const float* bias;
    int64_t b_mstride;
    const float* a;
    int64_t a_mstride;
    const float* h;
    int64_t h_mstride;
    float* out;
    int64_t o_mstride;
    int lda, ldh, ldo;
    int B, K, N, nnz;
    int mode, relu, out_rows, a_shared;
    int blocks, per_member;
    const float* dot_bias;                           /* nullable, with dot_acc: the bias path of the INPUT's layer */
    int64_t dot_b_mstride;
    float* dot_acc;
} lbbnn_sparse_gather_args_t;

typedef struct lbbnn_member_stats_args {
    const float* t;
    int64_t t_mstride;
    int ldt;
    int S, C, F, B;
    float *mean, *std, *prob_pos, *prob_neg, *members;
    const float* logits;
    int ldl, n_logits;
    const int64_t* targets;
    const float* intercept;
    float* residual;
} lbbnn_member_stats_args_t;

int lbbnn_sparse_draw_members(const lbbnn_sparse_draw_desc_t* layers, int n, int members, const uint64_t* rng, int flags,
                              void* stream);
int lbbnn_sparse_gather_members(const lbbnn_sparse_gather_args_t* args, void* stream);
int lbbnn_explain_seed(const float* logits, const int64_t* targets, int pred, int64_t* targets_out, const float* bias,
                       int64_t b_mstride, float* seed, int ld, float* intercept, int S, int B, int C, int Cp, uint64_t* rng_live,
                       uint64_t advance, void* stream);
int lbbnn_explain_member_stats(const lbbnn_member_stats_args_t* args, void* stream);

/* ------------------------------------------------------------------------------------------------------------------------------
 * Sparse median-probability model of a baseline LBBNN network (evaluate.freeze_base(net, "mpm", sparse=True)): the kept weights
 * of lbbnn_base_frozen_operands' LBBNN_GATES_MPM planes alone, in CSR, and every member's explicit weights drawn on that
 * pattern.  The baseline member IS an explicit-weight member (w = gate * (mu + sigma * eps), per weight), so one draw of
 * (members, nnz) values serves both the ensemble (lbbnn_sparse_gather_members, LBBNN_GATHER_FORWARD) and its explanation.
 * Per layer, columns ascending within a row:
 *     row_ptr (O + 1) int32, the exclusive scan of kept_rows;   col (nnz) int32;   mean (nnz) fp32 = weight_mu;
 *     sigma (nnz) fp32 = softplus(weight_rho);   b_mu (O) = bias_mu;   b_sigma (O) = softplus(bias_rho).
 * The keep rule is lbbnn_base_frozen_operands': sigmoid(lambdal) > threshold through its device functions, compared in fp32 (NaN
 * is never kept) -- NOT lambdal > logit(threshold), the rule of lbbnn_sparse_count, which can differ at the boundary: the pattern
 * is the dense frozen model's at every threshold.  sigma and not sigma^2 is stored (lbbnn_sparse_pack keeps var for the
 * local-reparameterisation sums): the draw multiplies by sigma, and sqrt(sigma^2) is not sigma to the bit.
 *
 * lbbnn_base_sparse_count: ONE launch for all n <= LBBNN_MAX_LAYERS layers, one wave per weight row: kept_rows[o] = the number of
 *   kept weights of row o.  Reads lambdal only; the caller scans kept_rows into row_ptr.
 *   NULL layers / lambdal / kept_rows: LBBNN_E_NULL; n outside [1, LBBNN_MAX_LAYERS], O <= 0, I <= 0: LBBNN_E_SHAPE; a threshold
 *   outside (0, 1): LBBNN_E_FLAGS; a pointer off a 4-B boundary: LBBNN_E_ALIGN.
 * lbbnn_base_sparse_pack: ONE launch for all n layers, one wave per weight row: 64 columns at a time the kept ones are compacted in
 *   ascending order (a ballot of the lanes and the count of the lower kept lanes give each its place) and col / mean / sigma are
 *   written from row_ptr[o] on, b_mu[o] and b_sigma[o] once per row.  Plain vector stores, no atomics.  Nothing is written at or
 *   past `nnz` (the capacity of col / mean / sigma) or past row_ptr[o + 1], whatever row_ptr holds.
 *   NULL layers / mu / rho / lambdal / bias_mu / bias_rho / row_ptr / b_mu / b_sigma, or col / mean / sigma with nnz > 0:
 *   LBBNN_E_NULL; the shapes above or nnz < 0: LBBNN_E_SHAPE; the threshold: LBBNN_E_FLAGS; a pointer off a 4-B boundary:
 *   LBBNN_E_ALIGN.
 *
 * lbbnn_base_sparse_draw_members: ONE launch for all n <= LBBNN_MAX_LAYERS layers and all members, one wave per CSR row (the
 *   members on gridDim.y with a stride inside).  Member m draws from {rng[0], rng[1] + m * member_advance}; with r the row of slot k
 *     w[m * w_mstride + k] = fmaf(sigma[k], eps, mean[k])     eps: stream LBBNN_STREAM_EPS_W * 64 + layer_id, counter
 *                            (r, col[k] / 4), word col[k] % 4 -- the weight's counter in the FULL network
 *     b[m * b_mstride + o] = fmaf(b_sigma[o], eps, b_mu[o])   eps: stream LBBNN_STREAM_EPS_B * 64 + layer_id, counter (o / 4, 0),
 *                            word o % 4
 *   which are, bit for bit, the weight (r, col[k]) and the bias o of member m of lbbnn_base_frozen_members in LBBNN_GATES_MPM mode
 *   from the same state (its mu + sigma * eps compiles to this one fused operation).  With tpos / wt (both or neither, else
 *   LBBNN_E_NULL) the value is stored once more at wt[m * w_mstride + tpos[k]], as lbbnn_sparse_draw_members does.
 *   LBBNN_F_MEAN_ONLY: w = mean, b = b_mu, nothing is drawn (rng may be NULL).  Every float of a member's block is written:
 *   w_mstride >= pad4(nnz), b_mstride >= pad4(O), the tail of the last 16-B quad is 0.  col is clamped into [0, I), tpos into
 *   [0, nnz), row_ptr into [0, nnz]: never followed outside.  A layer with nnz == 0 is legal (col / mean / sigma / w may be NULL).
 *   NULL layers, row_ptr / b_mu / b_sigma / b, or col / mean / sigma / w with nnz > 0: LBBNN_E_NULL; n outside [1,
 *   LBBNN_MAX_LAYERS], members outside [1, 65535], O < 1, I < 1, nnz < 0, a member stride below its padded row: LBBNN_E_SHAPE;
 *   flags other than 0 | LBBNN_F_MEAN_ONLY: LBBNN_E_FLAGS; rng == NULL without LBBNN_F_MEAN_ONLY: LBBNN_E_NOISE; w / wt / b off a
 *   16-B boundary or a stride of theirs not a multiple of 4, any other pointer off 4 B (rng: 8 B): LBBNN_E_ALIGN.  The caller
 *   advances rng afterwards. */
typedef struct lbbnn_base_sparse_desc {
    const float *mu, *rho, *lambdal;                 /* (O, I)                                  */
    const float *bias_mu, *bias_rho;                 /* (O)                                     */
    const int32_t* row_ptr;                          /* (O + 1); lbbnn_base_sparse_pack         */
    int32_t* col;                                    /* (nnz);   lbbnn_base_sparse_pack         */
    float *mean, *sigma;                             /* (nnz);   lbbnn_base_sparse_pack         */
    float *b_mu, *b_sigma;                           /* (O);     lbbnn_base_sparse_pack         */
    int32_t* kept_rows;                              /* (O);     lbbnn_base_sparse_count        */
    int O, I;
    int nnz;                                         /* capacity of col / mean / sigma          */
} lbbnn_base_sparse_desc_t;

typedef struct lbbnn_base_sparse_draw_desc {
    const int32_t *row_ptr, *col;                    /* (O + 1), (nnz)                          */
    const float *mean, *sigma;                       /* (nnz)                                   */
    const float *b_mu, *b_sigma;                     /* (O)                                     */
    const int32_t* tpos;                             /* (nnz) or NULL: place of slot k in wt    */
    float* wt;                                       /* [members][w_mstride] or NULL, with tpos */
    float* w;                                        /* [members][w_mstride]                    */
    int64_t w_mstride;
    float* b;                                        /* [members][b_mstride]                    */
    int64_t b_mstride;
    int O, I, nnz;
    uint32_t layer_id;
} lbbnn_base_sparse_draw_desc_t;

int lbbnn_base_sparse_count(const lbbnn_base_sparse_desc_t* layers, int n, float threshold, void* stream);
int lbbnn_base_sparse_pack(const lbbnn_base_sparse_desc_t* layers, int n, float threshold, void* stream);
int lbbnn_base_sparse_draw_members(const lbbnn_base_sparse_draw_desc_t* layers, int n, int members, const uint64_t* rng,
                                   uint64_t member_advance, int flags, void* stream);

/* ---- replicate study: R independent one-layer LRT fits in one launch (lrt_study.hip) ----
 *
 * lbbnn_lrt_study_fit: trains R one-layer LRT networks I -> O with a sigmoid head on BCELoss(sum) + kl * batch / N
 *   (LBBNN-GP-MF-MNFsim_study.py:305-395 with an LRT layer) for epochs first_epoch .. first_epoch + n_epochs - 1 in ONE
 *   launch: grid = R workgroups of 256 threads, replicate r is workgroup r.  A workgroup touches replicate r's slices only;
 *   there is no communication between workgroups (no atomics, no flags) and every loop bound is one of the counts below.
 *   An epoch is ceil(N / batch) steps over rows [k batch, min((k + 1) batch, N)) in order (the last batch may be short).
 *   State, loaded once, kept on chip for all steps of the launch, stored once (plain vector stores):
 *     params / exp_avg / exp_avg_sq  (R, 3 O I + 2 O): per replicate [weight_mu | weight_rho | lambdal | bias_mu | bias_rho]
 *     step (R) float Adam counters; rng (R, 2) {seed, offset}; skipped (R) running count of skipped steps.
 *   Step t of a replicate draws eps_out from philox_normal4 with state {seed, offset}, stream LBBNN_STREAM_EPS_OUT * 64 + 0,
 *   counter (b, o / 4), word o % 4, b the row INSIDE the batch -- layer l1 of a network -- and then offset += 1, skipped steps
 *   included.  alpha / sigma, the products, the head, the BCE term and its counts, the KL (LBBNN-GP-MF-LRT.py:185-194), the
 *   analytic backward and Adam use the expressions of weight_pass.hip, binary_head.hip, weight_pass_bwd.hip, vector_bwd.hip
 *   and adam.hip (hyper[r]: beta1, beta2, eps, coupled weight_decay; its lr and flags are not read).  Sums over rows have a
 *   fixed order: a replicate's bits depend on its own inputs only, and two launches of E / 2 epochs give the bits of one of E.
 *   lr: the rate of epoch e is lr[r * lr_rstride + e] (lr_rstride 0: one (epochs) table for all; else >= epochs).
 *   restarts: n_restarts epoch indices at whose start the moments and the step counter are zeroed (a re-created optim.Adam).
 *   x: (N, I) rows at x + r * x_rstride (0: shared); y: (N, O) floats at y + r * y_rstride; priors[r * priors_rstride]
 *   (priors_rstride 0 or 1).  All of these are DEVICE memory.
 *   Guard: a step whose fp32 loss is not finite, or whose batch has a probability that is not finite, changes no parameter,
 *   moment or step counter and adds 1 to skipped[r].
 *   history (R, epochs, 6) float64, row (r, e) written by workgroup r for the epochs of this launch: mean loss and mean nll
 *   over the steps that were not skipped (NaN without one), correct elements / elements, the last step's fp32 loss and its
 *   nll, skipped steps of the epoch.
 *   Checks, before the launch: a NULL struct or pointer (restarts with n_restarts > 0): LBBNN_E_NULL; I outside [1,
 *   LBBNN_STUDY_MAX_I], O outside [1, LBBNN_STUDY_MAX_O], O * I > LBBNN_STUDY_MAX_WEIGHTS, batch outside [1,
 *   LBBNN_STUDY_MAX_BATCH], N < 1, R outside [1, 65535], n_epochs < 0, first_epoch < 0, first_epoch + n_epochs > epochs,
 *   n_restarts < 0, a stride that is neither 0 nor at least its block: LBBNN_E_SHAPE; a pointer off 4 B (rng, skipped,
 *   history: 8 B): LBBNN_E_ALIGN.  n_epochs == 0: a successful no-op; otherwise ONE launch. */
#define LBBNN_STUDY_MAX_I 256
#define LBBNN_STUDY_MAX_O 16
#define LBBNN_STUDY_MAX_WEIGHTS 1024
#define LBBNN_STUDY_MAX_BATCH 4096
#define LBBNN_STUDY_HISTORY_COLS 6
typedef struct lbbnn_study_args {
    float *params, *exp_avg, *exp_avg_sq;            /* (R, 3 O I + 2 O)                        */
    float* step;                                     /* (R)                                     */
    uint64_t* rng;                                   /* (R, 2): {seed, offset}                  */
    int64_t* skipped;                                /* (R)                                     */
    const float* x;                                  /* (N, I) per replicate or shared          */
    int64_t x_rstride;
    const float* y;                                  /* (N, O) per replicate or shared          */
    int64_t y_rstride;
    const lbbnn_priors_t* priors;                    /* 1 or R rows                             */
    int priors_rstride;
    const lbbnn_adam_hyper_t* hyper;                 /* (R)                                     */
    const float* lr;                                 /* (epochs) or (R, lr_rstride)             */
    int64_t lr_rstride;
    const int32_t* restarts;                         /* (n_restarts) epoch indices, or NULL     */
    int n_restarts;
    double* history;                                 /* (R, epochs, 6)                          */
    int R, I, O, N, batch;
    int epochs, first_epoch, n_epochs;
} lbbnn_study_args_t;

int lbbnn_lrt_study_fit(const lbbnn_study_args_t* args, void* stream);

/* lbbnn_mnf_study_fit: the same launch for R one-layer planar-MNF networks I -> O with a sigmoid head (LBBNN-GP-MF-MNFsim_study.py
 *   with planar flows; lrt_study.hip, the MNF instantiation of the same kernel).  Everything said of
 *   lbbnn_lrt_study_fit holds -- one workgroup per replicate, no communication, fixed-order sums, the guard, the history --
 *   with these differences:
 *   Packed row (params / exp_avg / exp_avg_sq), the order of MNFBayesianLinear._param_list(), P = 3 O I + 2 O + 5 I +
 *   (Tz + Tr)(2 I + 1):
 *     [weight_mu | weight_rho | lambdal | bias_mu | bias_rho | q0_mean | q0_log_var | r0_c | r0_b1 | r0_b2 |
 *      z_flow t = 0 .. Tz - 1: u (I), w (I), b (1) | r_flow t = 0 .. Tr - 1 likewise]
 *   Draws of a step, Philox state {seed, offset}, layer id 0 -- the draws of layer l1 of an mnf.BayesianNetwork:
 *     eps_z[i], eps_z2[i]: streams LBBNN_STREAM_EPS_Z * 64 and LBBNN_STREAM_EPS_Z2 * 64, counter (i / 4, 0), word i % 4;
 *     eps_act[o]: stream LBBNN_STREAM_EPS_ACT * 64, counter (o / 4, 0), word o % 4; eps_out as lbbnn_lrt_study_fit; offset += 1.
 *   Forward (LBBNN-GP-MF-MNF.py:190-239): z_fwd = zflow(q0_mean + exp(q0_log_var / 2) eps_z), (z_kl, ldq) = zflow(.. eps_z2),
 *     (zb, ldr) = rflow(z_kl), the batch mean product over x * z_fwd, act_mu[o] = Sum_i r0_c z_kl mu alpha, act_var[o] =
 *     Sum_i r0_c^2 sigma^2 alpha^2, m = mean_o tanh(act_mu + sqrt(act_var) eps_act), kl = kl_bias + Sum kl_weight(mu z_kl)
 *     - ldq + log_q0 - ldr - log_rb (log_rb on zb's LAST element).  Tz = 0: z = z0, ldq = 0.
 *   Backward: weight_pass_bwd.hip's element chain with z_fwd, z_kl and the r0_c terms, vector_bwd.hip's V1 and V2.
 *   Adam over three rate groups -- 0: the ten named tensors, 1: z_flow, 2: r_flow -- with one step counter: the rate of group
 *   g in epoch e is lr[((r * lr_rstride) + e) * 3 + g] (lr_rstride 0: one (epochs, 3) table for all; else >= epochs).
 *   Checks as lbbnn_lrt_study_fit, in its order (NULL, shape, alignment); Tz or Tr outside [0, LBBNN_STUDY_MAX_TRANSFORMS]:
 *   LBBNN_E_SHAPE. */
#define LBBNN_STUDY_MAX_TRANSFORMS 4
typedef struct lbbnn_mnf_study_args {
    float *params, *exp_avg, *exp_avg_sq;            /* (R, P)                                  */
    float* step;                                     /* (R)                                     */
    uint64_t* rng;                                   /* (R, 2): {seed, offset}                  */
    int64_t* skipped;                                /* (R)                                     */
    const float* x;                                  /* (N, I) per replicate or shared          */
    int64_t x_rstride;
    const float* y;                                  /* (N, O) per replicate or shared          */
    int64_t y_rstride;
    const lbbnn_priors_t* priors;                    /* 1 or R rows                             */
    int priors_rstride;
    const lbbnn_adam_hyper_t* hyper;                 /* (R)                                     */
    const float* lr;                                 /* (epochs, 3) or (R, lr_rstride, 3)       */
    int64_t lr_rstride;
    const int32_t* restarts;                         /* (n_restarts) epoch indices, or NULL     */
    int n_restarts;
    double* history;                                 /* (R, epochs, 6)                          */
    int R, I, O, N, batch;
    int epochs, first_epoch, n_epochs;
    int Tz, Tr;                                      /* transforms of z_flow / r_flow, 0 .. 4   */
} lbbnn_mnf_study_args_t;

int lbbnn_mnf_study_fit(const lbbnn_mnf_study_args_t* args, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LBBNN_H_ */
