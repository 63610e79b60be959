/*
 * nsfnet_pinn.h - C ABI of the MI355X (gfx950) PINN training-step library.
 *
 * The reference (latteine1217/NSFnet) has no FFI: its hot path is Python calling
 * torch autograd.  This header is the boundary a maintainer binds instead of that
 * path; every entry point names the reference code it replaces.  All pointers are
 * DEVICE pointers owned by the caller (e.g. PyTorch's allocator); the library never
 * allocates or frees device memory, launches only on the stream it is given, spawns
 * no threads and keeps no global mutable state besides the last-error string.
 * Return value: 0 on success, negative on error (see pinn_last_error()).
 *
 * Parameters of a network are ONE flat fp32 vector in torch state_dict order of the
 * reference FCNet (NSFnet/net.py:36-46):
 *   layers.layer_0.weight (H,2) | layers.layer_0.bias (H) | layers.layer_l.weight (H,H) |
 *   layers.layer_l.bias (H) ... | layers.layer_L.weight (n_out,H) | layers.layer_L.bias (n_out)
 * so reference checkpoints map onto it by concatenation.
 */
#ifndef NSFNET_PINN_H
#define NSFNET_PINN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pinn_net_s* pinn_net_t;
typedef struct pinn_plan_s* pinn_plan_t;

/* field planes written by pinn_residual_forward (plane stride = pinn_plan_padded_points) */
enum {
  PINN_FLD_U = 0, PINN_FLD_V, PINN_FLD_UX, PINN_FLD_UY, PINN_FLD_VX, PINN_FLD_VY,
  PINN_FLD_EQ1, PINN_FLD_EQ2, PINN_FLD_EQ3, PINN_FLD_EQ4, PINN_FLD_P, PINN_FLD_COUNT
};
#define PINN_NLOSS 8

const char* pinn_last_error(void);
/* 3 = this header (2 + pinn_plan_kernel; 2 = 1 + pinn_adam_step_dev, bf16 modes for every width up to 512). */
int pinn_abi_version(void);

/* ---- network description --------------------------------------------------
 * Replaces FCNet.__init__ (NSFnet/net.py:23-50): 2 inputs, `n_hidden_layers` tanh
 * layers of width `hidden`, `n_out` linear outputs (3 = u,v,p ; 1 = entropy residual e).
 * hidden <= 512. */
int pinn_net_create(int n_out, int n_hidden_layers, int hidden, pinn_net_t* out);
int pinn_net_destroy(pinn_net_t net);
/* Arithmetic of the three MFMA kernel families (forward sweep, reverse sweep, weight-gradient
 * GEMM): 0 = f32-input MFMA (bit-exact fp32 fmaf chains, default), 1 = bf16x3 (fp32 operands
 * split into bf16 hi+lo, three bf16 MFMAs per product, fp32 accumulate; ~2^-17 relative per
 * product), 2 = plain bf16 operands (fast mode, does NOT meet the 1e-4 loss-parity bar).
 * All three modes exist for every supported width (hidden <= 512).  Call before pinn_net_prepare / pinn_plan_create. */
int pinn_net_set_precision(pinn_net_t net, int prec_fwd, int prec_bwd, int prec_dw);
/* ---- frozen Fourier-feature first layer (opt-in) ---------------
 * The random-Fourier-feature embedding gamma(x) = [cos(2 pi B x), sin(2 pi B x)], B of shape (hidden / 2) x 2, followed
 * by a tanh MLP, is this net with two changes: layer 0 uses sin instead of tanh, and layer 0 is frozen.  Rows 2k and
 * 2k + 1 of W0 both hold 2 pi B_k, their biases are pi / 2 (the cosine) and 0 (the sine); the caller writes them into
 * the flat parameters, whose keys and shapes do not change.  With kind = PINN_FIRST_LAYER_SINE, for the coordinates
 * the net is fed:
 *     z   = fmaf(w0x, x, fmaf(w0y, y, b0))                                  (as before)
 *     a   = sin z     a_x = cos z * w0x     a_y = cos z * w0y     a_D = -sin z * (w0x^2 + w0y^2)
 * (value mode: a alone); layers 1 .. L-1 and the output layer are exactly what they are with tanh.  fp32 mode uses the
 * accurate sinf / cosf, the bf16 modes the hardware sine and cosine after an explicit range reduction.
 * Layer 0 is not trained: its 3 * hidden gradient entries - the first 3 * hidden of the flat vector - are +0.0 bit for
 * bit in every vector that pinn_grad_reduce, pinn_grad_reduce_terms and pinn_grad_reduce_terms_gram write (the
 * statistics and Gram partials see the zeros), whether or not the call accumulates.
 * The kind belongs to the net: every plan over it (residual, value) sees the same function.  A plan keeps the kind
 * its net had when it was created; after a change every launch on such a plan, and every gradient assembly from it,
 * is refused by name - create the plan again.
 * By default plans of such a net run the 8-wave kernel families whatever PINN_SCHED / PINN_WSPLIT / PINN_FUSE say, and
 * store layer 0 (its a-streams) whatever PINN_S0_SKIP32 says; pinn_plan_kernel names the kernels as before.  With
 * PINN_FF_SPLIT=1 in the environment when a residual (4-stream) plan is created it keeps the role-split (hidden 256),
 * fused and wide role-split (hidden 288 .. 448) sweeps that PINN_SCHED, PINN_FWD_SCHED, PINN_BWD_SCHED, PINN_WSPLIT and
 * PINN_FUSE give a tanh net's plan - the same names, workspace bytes and padded points - in variants whose forward forms
 * layer 0 by the lines above and whose reverse sweep, the layer being frozen, ends at layer 1.  Only whole plans: where
 * either sweep would run the pipelined schedule or an 8-wave kernel (PINN_SCHED=1, one role-split sweep without the
 * other, an fp32 dW, PINN_WSPLIT=0, hidden 480 or 512, LDS) the plan is exactly the default one.  The fused kernel
 * computes bit for bit what the two launches compute.  Forward-only calls (save = 0), value plans and the fp32 mode run
 * the 8-wave variant either way.  No other plan looks at PINN_FF_SPLIT, and such a plan never looks at PINN_HBC_SPLIT or
 * PINN_PTIME_SPLIT.
 * Refused (-22, pinn_last_error names the reason): an odd hidden width; fewer than 2 hidden layers (the output
 * layer's gradient is formed from the last hidden layer by the tanh rule); pinn_plan_create_constrained with walls
 * and pinn_plan_create_pseudo_time over such a net. */
enum { PINN_FIRST_LAYER_TANH = 0, PINN_FIRST_LAYER_SINE = 1 };
int pinn_net_set_first_layer(pinn_net_t net, int kind);
int pinn_net_first_layer(pinn_net_t net);      /* the kind; -1 for a null net */
int64_t pinn_net_num_params(pinn_net_t net);
int64_t pinn_net_prep_floats(pinn_net_t net);
/* Re-layout the flat parameters into padded MFMA-fragment order; call after every
 * parameter update.  (No reference counterpart: torch re-reads nn.Linear weights.) */
int pinn_net_prepare(pinn_net_t net, const float* params, float* prep, void* stream);

/* ---- plan: `n_points` points evaluated by `net` ------------------------------
 * streams = 4: residual mode (value, d/dx, d/dy, Laplacian)  - collocation points
 * streams = 1: value mode                                    - boundary / supervised /
 *                                                              evaluation points, entropy net */
int pinn_plan_create(pinn_net_t net, int64_t n_points, int streams, pinn_plan_t* out);
int pinn_plan_destroy(pinn_plan_t plan);
int64_t pinn_plan_padded_points(pinn_plan_t plan);
int64_t pinn_plan_workspace_bytes(pinn_plan_t plan, int with_backward);
/* Name of the kernel family the plan launches for `which` = 0 forward (with saved activations), 1 reverse sweep,
 * 2 weight-gradient GEMM - what appears in a rocprofv3 kernel trace (e.g. "fwd_pipe_kernel", "bwd_bf16_kernel").
 * For profiling harnesses (bench.py keys its roofline / PMC lookup on it); static string, never NULL for a valid plan. */
const char* pinn_plan_kernel(pinn_plan_t plan, int which);

/* ---- residual forward -------------------------------------------------------
 * Replaces neural_net_equations + the PDE half of fwd_computing_loss_2d
 * (NSFnet/pinn_solver.py:132-163,212-222; ev-NSFnet/pinn_solver.py:290-342,384-397).
 *   x,y          [n] collocation coordinates
 *   e            [n] entropy-net output (ev flavour) or NULL (plain NSFnet: eq4 = 0)
 *   w            [n] per-point weights (SDF weights, ev:387-392) or NULL
 *   vis_t_minus  [n] in/out lagged viscosity state alpha_evm*|e_prev| (ev:327-334) or NULL
 *   vis_t_out    [n] out: artificial viscosity min(vis_t0, vis_t_minus) used this call, or NULL
 *   fields       [PINN_FLD_COUNT][padded] out: u,v,u_x,u_y,v_x,v_y,eq1..eq4,p
 *   loss_sums    [PINN_NLOSS] out: sum_i w_i eq_k,i^2 for k=1..4 in slots 0..3
 *   save != 0 keeps the activations in `ws` for pinn_residual_backward. */
int pinn_residual_forward(pinn_plan_t plan, void* ws, const float* prep,
                          const float* x, const float* y, const float* e, const float* w,
                          float* vis_t_minus, float* vis_t_out, float* fields,
                          float Re, float vis_t0, float alpha_evm, float coord_scale,
                          int save, float* loss_sums, void* stream);

/* ---- residual backward ------------------------------------------------------
 * Replaces loss.backward() for the PDE loss (NSFnet/pinn_solver.py:252; ev:469):
 * d/dtheta of sum_k coef_eq[k]/2 * sum_i w_i eq_k,i^2, i.e. the caller passes
 * coef_eq[k] = 2*alpha_e*c_k/N_global (c = 1,1,1,0.1).  Partial gradients stay in `ws`
 * until pinn_grad_reduce.  ebar_out [n] (or NULL) receives d loss/d e.
 * coef_eq4 is a HOST array of 4 floats. */
int pinn_residual_backward(pinn_plan_t plan, void* ws, const float* prep,
                           const float* x, const float* y, const float* e, const float* w,
                           const float* vis_t, const float* fields, const float* coef_eq4,
                           float Re, float coord_scale, float* ebar_out, void* stream);

/* Same, restricted to phases (bit 0: adjoint sweep that spills the z-adjoints, bit 1:
 * weight-gradient GEMM); for per-kernel timing in bench.py.  phases = 3 is the call above. */
int pinn_residual_backward_phases(pinn_plan_t plan, void* ws, const float* prep,
                                  const float* x, const float* y, const float* e, const float* w,
                                  const float* vis_t, const float* fields, const float* coef_eq4,
                                  float Re, float coord_scale, float* ebar_out, int phases, void* stream);

/* ---- residual forward + backward in one call ------------------------------
 * pinn_residual_forward(save = 1) followed by pinn_residual_backward (MSE seeds coef_eq4,
 * known before the forward), with the same arguments and the same results: fields,
 * vis_t_out, vis_t_minus, loss_sums, ebar_out and the partial gradients for
 * pinn_grad_reduce.  On the role-split hidden-256 plan the two sweeps of each tile run
 * in one kernel (PINN_FUSE=0 at plan creation keeps the separate launches); on every
 * other plan this is exactly the two calls.  Not for seeds that depend on the loss sums
 * (the L2 loss mode). */
int pinn_residual_forward_backward(pinn_plan_t plan, void* ws, const float* prep,
                                   const float* x, const float* y, const float* e, const float* w,
                                   float* vis_t_minus, float* vis_t_out, float* fields,
                                   const float* coef_eq4, float Re, float vis_t0, float alpha_evm,
                                   float coord_scale, float* loss_sums, float* ebar_out, void* stream);

/* ---- value forward / backward -----------------------------------------------
 * Replaces neural_net_u and the boundary / supervised MSE terms
 * (NSFnet/pinn_solver.py:124-130,199-207; ev:280-288,374-379,399-411) and, with
 * save = 0, the inference forward of evaluate/test (NSFnet/pinn_solver.py:308-357).
 *   pred3/tgt3/coef3 are HOST arrays of 3 entries (device pointers / floats):
 *   pred[c]  [n] out planes or NULL ; tgt[c] [n] targets or NULL (NaN target = masked)
 *   coef[c]  output adjoint scale: oadj_c = coef[c]*(pred_c - tgt_c), kept in ws
 *   loss_sums slots 0..2 = sum (pred_c - tgt_c)^2 over valid targets, slot 3 = number
 *   of valid targets of output 2. */
int pinn_value_forward(pinn_plan_t plan, void* ws, const float* prep,
                       const float* x, const float* y,
                       float* const* pred3, const float* const* tgt3, const float* coef3,
                       int save, float* loss_sums, void* stream);
/* out_adj: [n_out][padded] explicit output adjoints, or NULL to use the ones
 * pinn_value_forward left in ws. */
int pinn_value_backward(pinn_plan_t plan, void* ws, const float* prep,
                        const float* x, const float* y, const float* out_adj, void* stream);

/* ---- gradient assembly, optimizer -------------------------------------------
 * Sum the partial gradients of up to 4 (plan, ws) pairs of the SAME net into the flat
 * gradient (state_dict order), fixed summation order. */
int pinn_grad_reduce(pinn_net_t net, int nsrc, const pinn_plan_t* plans, void* const* wss,
                     float* grads, int accumulate, void* stream);
/* torch.optim.Adam step (NSFnet/pinn_solver.py:76-79,253; ev:126-129,472); step >= 1. */
int pinn_adam_step(float* params, const float* grads, float* m, float* v, int64_t n,
                   float lr, float beta1, float beta2, float eps, int64_t step, void* stream);

/* Same update with the step count in DEVICE memory: step_counter points at TWO int64 words, [0] = steps taken
 * so far, [1] = scratch that must be zero on entry (both zero to start / restart the schedule).  The call uses
 * t = step_counter[0] + 1 for the bias corrections and increments step_counter[0] when its last workgroup is
 * done, so a whole training step can be captured in a hipGraph and replayed with no host-side scalar changing
 * between steps. */
int pinn_adam_step_dev(float* params, const float* grads, float* m, float* v, int64_t n,
                       float lr, float beta1, float beta2, float eps, int64_t* step_counter, void* stream);

/* ---- residual-based resampling of the collocation points (RAD) -----------------
 * No reference counterpart (its roadmap asks for finer control of the PDE points,
 * ev-NSFnet/README.md).  A pool of n_pool candidate points evaluated by a forward-only
 * residual plan (its fields, plane stride npad) is resampled to m points by systematic
 * resampling, all sums in fp64 and in a fixed order (bit-reproducible):
 *   e2_i = eq1^2 + eq2^2 + eq3^2 + w4 eq4^2,  a_i = e2_i^(k/2)  (k = 0: 1; k = 1: sqrt; k = 2: e2_i;
 *          k = 0 with a non-finite e2_i: NaN, so that a non-finite residual always shows in S)
 *   S = sum a_i (S == 0: a_i = 1),  b_i = a_i + c S / n_pool,  C_i = inclusive prefix sum of b,
 *   T = C_{n_pool-1},  o_i = min(m, floor(C_i m / T + u)),  o_{-1} = 0,  o_{n_pool-1} = m,
 *   pool point i is written to out[o_{i-1} .. o_i).
 * out is ascending (the selection keeps the pool order) and a point may appear more than once.
 *
 * Limits: 1 <= n_pool <= 2^30 and 1 <= m <= 2^30 (as for a plan's points).
 *
 * Bytes of device scratch the two calls below need for a pool of n_pool points (-1 if n_pool is out of range). */
int64_t pinn_resample_scratch_bytes(int64_t n_pool);
/* out [m] int64 pool indices.  After the call the first 8 bytes of scratch hold S (fp64), for the
 * caller to check (a non-finite S means a non-finite residual in the pool).  k, c, w4 >= 0 and
 * finite, 0 <= u < 1; fields 16-byte aligned, npad >= n_pool and a multiple of 4. */
int pinn_resample_select(int64_t n_pool, const float* fields, int64_t npad, double w4, double k, double c,
                         double u, int64_t m, void* scratch, int64_t* out, void* stream);
/* dst_*[j - lo] = src_*[idx[j]] for j in [lo, hi) (0 <= lo < hi; indices outside [0, n_pool) are skipped): x and y always, w and vis_t_minus when both
 * their source and destination are non-NULL.  w_sum (device, one double, or NULL; needs w)
 * receives the fp64 sum of the gathered w in a fixed order.  scratch as for the select call
 * with the same n_pool (its first 8 bytes are left alone). */
int pinn_resample_gather(const int64_t* idx, int64_t lo, int64_t hi, int64_t n_pool,
                         const float* src_x, const float* src_y, const float* src_w, const float* src_vtm,
                         float* dst_x, float* dst_y, float* dst_w, float* dst_vtm,
                         void* scratch, double* w_sum, void* stream);

/* ---- L-BFGS direction (compact representation) --------------------------------------
 * No reference counterpart (its authors' next step: "L-BFGS integration in Stage 3",
 * ev-NSFnet/AGENTS.md:73).  The device half of torch.optim.LBFGS.step: the history of pairs
 * s = t_prev d_prev, y = g - g_prev, the inverse-Hessian direction d = -H g and the scalars the
 * host-side line search needs.  A pair enters only if y's > 1e-10; once `history` pairs are held
 * the oldest is dropped; gamma (H0 = gamma I) is y's / y'y of the newest accepted pair.  With
 * S = [s_0 .. s_k-1], Y likewise (oldest first), R_ij = s_i'y_j (i <= j), D = diag(s_i'y_i),
 * a = S'g, b = Y'g (Byrd, Nocedal & Schnabel 1994):
 *   u = R^-1 a ,  p = R^-T ((D + gamma Y'Y) u - gamma b) ,  d = -(gamma g + S p - gamma Y u)
 * which equals the two-loop recursion.  All sums are fp64 in a fixed order (no atomics): the result
 * is bit-reproducible, and ranks that hold the same g compute the same d and scalars.
 *
 * Vectors: n fp32 entries, g and d 16-byte aligned.  history: 1..PINN_LBFGS_MAX_HISTORY.  The
 * workspace (256-byte aligned, pinn_lbfgs_workspace_bytes; -1 for bad sizes) holds history + 1
 * slots of s and y (a rejected pair never overwrites a live one), g_prev, R and Y'Y in fp64 and
 * the reduction partials.  result: 8 doubles (device). */
#define PINN_LBFGS_MAX_HISTORY 1024
int64_t pinn_lbfgs_workspace_bytes(int64_t n, int history);
/* Empty history.  The next pinn_lbfgs_direction must pass t_prev = 0. */
int pinn_lbfgs_reset(void* ws, int64_t n, int history, void* stream);
/* One iteration's direction at gradient g.  t_prev = 0: no pair (first iteration, or after a
 * reset): the history is emptied, gamma = 1 and d = -g.  Otherwise d holds the previous direction
 * on entry and the pair (t_prev d, g - g_prev) is offered to the history first; t_prev < 0 offers
 * the pair of a zero step (s = 0: rejected, history and gamma kept, as torch does after a line
 * search that accepted t = 0).  On return d is
 * the new direction, g_prev = g, and
 *   result[0] = g'd   [1] = max|d|   [2] = sum|g|   [3] = max|g|   (max: NaN-propagating)
 *   result[4] = 1 accepted / 0 rejected / -1 first   [5] = pairs held   [6] = gamma   [7] = y's */
int pinn_lbfgs_direction(void* ws, int64_t n, int history, const float* g, float t_prev, float* d, double* result,
                         void* stream);
/* Line-search probe at a trial gradient g against direction d: result[0..3] as above. */
int pinn_lbfgs_probe(void* ws, int64_t n, int history, const float* g, const float* d, double* result, void* stream);

/* ---- adaptive loss-weight balancing ----------------------------------------------------
 * No reference counterpart: the "dynamic weights" of the NSFnets line of work, i.e. the learning-rate-
 * annealing rule of Wang, Teng & Perdikaris (2021, Algorithm 1).  For the main net's P parameters:
 *   g_r = grad(alpha_e L_e)  (residual loss, as today)   g_b = grad L_b  (boundary, unit weight)
 *   g_s = grad L_s  (supervised, unit weight; only when that loss is active), all global (summed over ranks).
 * On a balance step, for each weighted term t (b, and s when active):
 *   lambda_hat_t = max_j |g_r,j| / ((1/P) sum_j |g_t,j|),   lambda_t <- (1 - beta) lambda_t + beta lambda_hat_t
 * and if lambda_hat_t is not finite or its denominator is 0, lambda_t keeps its value and the skip count goes up by
 * one.  The gradient Adam consumes is g = g_r + lambda_b g_b + lambda_s g_s.  The weights live on the device; the
 * host never reads them on the step path.  All sums are fp64 in a fixed order, no float atomics: the results are
 * bit-reproducible, and ranks that hold the same vectors compute the same weights.
 *
 * Statistics travel in per-block partials: for every block of 64 consecutive parameters b and term t (0 = r,
 * 1 = b, 2 = s), partials[6 b + 2 t] = max|g_t| over the block (NaN-propagating) and [6 b + 2 t + 1] = sum|g_t|.
 * Doubles of partials for n parameters: */
int64_t pinn_balance_partials_count(int64_t n);
/* The gradient assembly of pinn_grad_reduce with the sources in three consecutive groups: nsrc3[0] collocation
 * sources, then nsrc3[1] boundary and nsrc3[2] supervised ones (host array of 3; total 1..4).  Each group is summed
 * in the same fixed fp64 order as pinn_grad_reduce into its own fp32 vector out3[t] (host array of 3 device pointers).
 * out3[t] NULL: group t not written (needs nsrc3[t] = 0).  nsrc3[t] = 0 with out3[t] given: zeros are written.
 * Bit t of accumulate_mask adds to out3[t] instead.  partials (device, or NULL): the partials above of the values
 * written (0 for a group not written). */
int pinn_grad_reduce_terms(pinn_net_t net, const int* nsrc3, const pinn_plan_t* plans, void* const* wss,
                           float* const* out3, int accumulate_mask, double* partials, void* stream);
/* The partials of three device vectors of n entries (vec3: host array of 3 device pointers; NULL = zeros). */
int pinn_balance_stats(const float* const* vec3, int64_t n, double* partials, void* stream);
/* One balance update from the partials of n parameters (one workgroup).  terms: bit 0 = update lambda_b, bit 1 =
 * update lambda_s.  0 < beta <= 1.  record: PINN_BALANCE_RECORD doubles (device) that hold the state,
 *   [0] max|g_r| [1] mean|g_r| [2] max|g_b| [3] mean|g_b| [4] lambda_hat_b [5] max|g_s| [6] mean|g_s|
 *   [7] lambda_hat_s (0 for a term not updated) [8] skipped term updates [9] lambda_b [10] lambda_s
 *   [11] balance updates made;
 * the caller initialises [8] = [11] = 0 and [9], [10] to the configured weights.  lam (device, 2 floats) receives
 * (float) lambda_b, (float) lambda_s. */
#define PINN_BALANCE_RECORD 12
int pinn_balance_update(const double* partials, int64_t n, int terms, double beta, float* lam, double* record,
                        void* stream);
/* g = g_r + lam[0] g_b + lam[1] g_s (fp32 fused multiply-adds in that order; gs NULL: no supervised term).  g may be
 * g_r. */
int pinn_balance_combine(float* g, const float* gr, const float* gb, const float* gs, const float* lam, int64_t n,
                         void* stream);

/* ---- conflict-free combination of the per-term gradients --------------------------------
 * No reference counterpart: ConFIG (Liu, Chu & Thuerey, "ConFIG: Towards Conflict-free Training of Physics Informed
 * Neural Networks", ICLR 2025), the stateless alternative to the balancing above.  With g_t the global gradient of
 * loss term t of the main net's P parameters, weights baked in (r = alpha_e L_e, b = alpha_b L_b, s = alpha_s L_s;
 * m = 2 terms, or 3 with the supervised loss), the gradient Adam consumes is the one with equal positive projection
 * on every term's unit gradient, its length the sum of the terms' projections on it:
 *   A_ij = g_i . g_j    n_t = sqrt(A_tt)    M_ij = A_ij / (n_i n_j)    solve M c = 1
 *   k_t = (sum_i n_i / sum_i c_i) c_t / n_t                           g = sum_t k_t g_t
 * (two terms: k_t = (n_r + n_b) / (2 n_t)).  There is no state besides counters.  Guards, decided on the device:
 * a term with n_t = 0 leaves the set (one term left: g is that term, k = 1; none: g = 0, k = 0); a non-finite Gram
 * entry, det(M) <= 1e-10, sum c <= 0 or a non-finite c_t make the step fall back to the plain sum k = (1, 1, 1),
 * which is the gradient without this feature.  All sums are fp64 in a fixed order, no float atomics: the results
 * are bit-reproducible, and ranks that hold the same vectors compute the same coefficients.
 *
 * Statistics travel in per-block partials: for every block b of 64 consecutive parameters, partials[6 b + 0..5] =
 * the dot products rr, bb, ss, rb, rs, bs over the block (exact fp64 products of the fp32 entries).  Doubles of
 * partials for n parameters (= pinn_balance_partials_count; -1: n outside 1..2^30): */
int64_t pinn_confgrad_partials_count(int64_t n);
/* pinn_grad_reduce_terms that also writes the Gram partials of the three vectors it wrote (an unwritten group counts
 * as zeros) to gram_partials (device, or NULL: exactly pinn_grad_reduce_terms).  One launch either way. */
int pinn_grad_reduce_terms_gram(pinn_net_t net, const int* nsrc3, const pinn_plan_t* plans, void* const* wss,
                                float* const* out3, int accumulate_mask, double* partials, double* gram_partials,
                                void* stream);
/* The Gram partials of three device vectors of n entries (vec3: host array of 3 device pointers; NULL = zeros). */
int pinn_confgrad_gram(const float* const* vec3, int64_t n, double* partials, void* stream);
/* The coefficients from the partials of n parameters (one workgroup).  nterms: 2 (r, b) or 3 (r, b, s).  coef
 * (device, 3 floats) receives (float) k_r, k_b, k_s.  record: PINN_CONFGRAD_RECORD doubles (device),
 *   [0] n_r [1] n_b [2] n_s   [3] cos_rb [4] cos_rs [5] cos_bs (0 for a pair outside the set)   [6] k_r [7] k_b [8] k_s
 *   [9] |g| = sum n / sqrt(sum c) (fallback: the norm of the plain sum)
 *   [10] steps made   [11] fallbacks   [12] terms dropped for a zero norm (counted per step and term);
 * [0..9] are overwritten, [10..12] accumulate: the caller zeroes them to start. */
#define PINN_CONFGRAD_RECORD 13
int pinn_confgrad_coef(const double* partials, int64_t n, int nterms, float* coef, double* record, void* stream);
/* g = coef[0] g_r + coef[1] g_b + coef[2] g_s: one fp32 product, then fp32 fused multiply-adds in that order (gs
 * NULL: no supervised term).  g may be g_r. */
int pinn_confgrad_combine(float* g, const float* gr, const float* gb, const float* gs, const float* coef, int64_t n,
                          void* stream);

/* ---- stochastic mini-batching of the collocation term ---------------------------------
 * No reference counterpart (its roadmap asks for "mini-batch PDE points", ev-NSFnet/README.md; its `batchsize`
 * argument is dead).  A store of n collocation points (x, y, optional weights w, optional lagged state vis_t_minus)
 * stays resident; every call draws a batch of b points from it (1 <= b <= n <= 2^30), stratified, one point per
 * stratum, all in integers.  For batch slot j in [0, b):
 *   lo = floor(j n / b),  hi = floor((j + 1) n / b)                      (64-bit arithmetic)
 *   r  = word 0 of Philox4x32-10, counter (j_lo32, j_hi32, t_lo32, t_hi32), key (seed_lo32, rank)
 *   idx[j] = lo + ((r * (hi - lo)) >> 32)                                (32 x 32 -> 64-bit product, high word)
 *   dst_*[j] = src_*[idx[j]]   for x and y, and for w / vis_t_minus where given
 * idx is strictly ascending (an ordering of the store survives) and b = n draws the identity.  When b does not
 * divide n the strata differ by one point, so a point's inclusion probability differs by that much.
 * t is the draw counter counter[0] in DEVICE memory: the draw reads it and advances it by one when every workgroup
 * is done, so a captured hipGraph draws a new batch on every replay with no host scalar changing.  counter: two
 * int64, [0] = t, [1] = scratch that is 0 between calls; the caller zeroes both to restart the sequence.
 * src_w and dst_w (and src_vtm and dst_vtm) are both given or both NULL = absent.  The batch buffers must not
 * overlap the store.  One launch. */
int pinn_batch_draw(int64_t n, int64_t b, uint64_t seed, int rank, int64_t* counter,
                    const float* src_x, const float* src_y, const float* src_w, const float* src_vtm,
                    float* dst_x, float* dst_y, float* dst_w, float* dst_vtm, int64_t* idx, void* stream);
/* store_vtm[idx[j]] = batch_vtm[j] for j in [0, b): the batch's updated lagged state back to the store (ev flavour).
 * idx as written by pinn_batch_draw: distinct, so no atomics; an index outside [0, n) is skipped.  Nothing else of
 * the store is written.  One launch. */
int pinn_batch_scatter(const int64_t* idx, int64_t b, int64_t n, const float* batch_vtm, float* store_vtm,
                       void* stream);

/* ---- residual-based attention weights on the collocation points -----------------------
 * No reference counterpart (its roadmap asks for finer control of the PDE points, ev-NSFnet/README.md).  Residual-based
 * attention (RBA; Anagnostopoulos, Toscano, Stergiopulos & Karniadakis 2024): every collocation point of the resident
 * store carries a multiplier that grows where the residual stays large and decays where it does not.  State per
 * local store point i (n_store of them):
 *   lam [n_store] fp32   the attention multiplier
 *   s   [n_store] fp32   the static weights (SDF weights); NULL = 1
 *   w   [n_store] fp32   the effective weight the residual kernels read, w_i = s_i lam_i^2
 * After an evaluation has written the UNWEIGHTED residual planes eq1..eq4 of its n points (the planes
 * pinn_resample_select reads), with i = idx[j], or i = j without idx:
 *   e2_j   = eq1^2 + eq2^2 + eq3^2 + w4 eq4^2      (w4 = the eq4 weight of the ev flavour, 0 for plain NSFnet)
 *   r_j    = sqrt(e2_j)
 *   rmax   = max_j r_j                              (NaN-propagating; over the points of ALL ranks)
 *   lam_i <- gamma lam_i + eta r_j / rmax
 *   w_i   <- s_i lam_i^2
 * Every per-point value is computed in fp64 from the fp32 inputs, without contraction, in exactly this order
 * (((eq1^2 + eq2^2) + eq3^2) + w4 eq4^2; gamma lam + (eta r) / rmax), and rounded to fp32 once on store; w is
 * s (lam lam) of the STORED fp32 lam, rounded once, so w is always a function of the stored s and lam.  If rmax is
 * not finite or is 0 nothing is written and the record's skip count goes up by one (the convention of
 * pinn_balance_update).  0 < gamma <= 1, eta >= 0; lam stays within [0, max(lam_0, eta / (1 - gamma))].
 *
 * Two calls, so that a caller with several ranks can place a MAX all-reduce of the one rmax word between them.
 * scratch: pinn_rba_scratch_bytes(n) bytes of device memory, 8-byte aligned, ZERO before the first call (both calls
 * leave their workgroup tickets 0); sized for the largest n it is used with.  One scratch serves one stream at a
 * time.  As doubles: [0] rmax - a NaN is stored
 * as the positive quiet NaN, so the signed-integer order of the eight bytes is the NaN-propagating order of the
 * values and an int64 MAX all-reduce of that word gives the global rmax; [1..4] the fp64 sums of eq1^2 .. eq4^2
 * over the n points; then tickets and block partials.  Bytes of scratch for evaluations of up to n points
 * (-1: n outside 1..2^30): */
int64_t pinn_rba_scratch_bytes(int64_t n);
/* rmax and the four unweighted sums of the n points of `fields` ([PINN_FLD_COUNT][npad] fp32, 16-byte aligned, npad a
 * multiple of 4 and >= n) into scratch[0..4]; w4 = 0: the eq4 plane is not read and its sum is 0.  One launch: a grid-stride loop of 16-byte loads, wave reduction by
 * shuffles, per-block partials, and the last block to finish folds them in block order.  No float atomics: every
 * sum has a fixed order and the result is bit-reproducible. */
int pinn_rba_stats(int64_t n, const float* fields, int64_t npad, double w4, double* scratch, void* stream);
/* The update above with rmax = scratch[0].  idx: NULL, or the n int64 store indices of the evaluation's points as
 * written by pinn_batch_draw (distinct, so no atomics; an index outside [0, n_store) is skipped); without idx
 * n <= n_store.  s: NULL = 1.  lam, w (and s) must be 16-byte aligned.  record: PINN_RBA_RECORD doubles (device),
 *   [0] rmax  [1..4] the sums of eq1^2 .. eq4^2 of this evaluation (scratch[1..4])
 *   [5] min [6] max [7] sum of the lam values written by the last update (fp64, fixed order)  [8] their count
 *   [9] updates made  [10] updates skipped  [11] 0;
 * the caller zeroes it once; a skipped update rewrites [0..4] and [10] only.  One launch. */
#define PINN_RBA_RECORD 12
int pinn_rba_apply(int64_t n, const float* fields, int64_t npad, double w4, double gamma, double eta,
                   const int64_t* idx, int64_t n_store, const float* s, float* lam, float* w, double* scratch,
                   double* record, void* stream);
/* lam_i = init, w_i = s_i init^2 for the n store points (s NULL = 1; init >= 0).  One launch. */
int pinn_rba_fill(int64_t n, double init, const float* s, float* lam, float* w, void* stream);

/* ---- learning-rate schedules and global-norm gradient clipping for Adam ----------------
 * The reference documents a per-stage `scheduler` key (Constant | MultiStepLR | CosineAnnealingLR,
 * ev-NSFnet/AGENTS.md:44,66) that steps a torch.optim.lr_scheduler on the host.  Here the schedule position is an
 * epoch counter e in DEVICE memory, like the step count of pinn_adam_step_dev, and the learning rate of epoch e is
 * computed inside the update kernel from launch constants, so one captured step serves a whole stage.  e is a counter
 * of its own, not Adam's t: re-creating Adam (t = 0, zero moments) leaves the schedule position alone.
 *
 * lr_e, in fp64, from lr0 and a pinn_lr_schedule_t s (the closed forms of torch.optim.lr_scheduler):
 *   PINN_LR_CONSTANT     lr0
 *   PINN_LR_MULTISTEP    lr0 gamma^k,  k = number of the n_milestones (<= PINN_LR_MAX_MILESTONES) milestones <= e
 *   PINN_LR_STEP         lr0 gamma^floor(e / step_size)
 *   PINN_LR_EXPONENTIAL  lr0 gamma^e
 *   PINN_LR_COSINE       eta_min + (lr0 - eta_min) (1 + cos(pi e / t_max)) / 2      (continues past t_max)
 * times, when W = warmup_epochs > 0, the linear warm-up factor warmup_start + (1 - warmup_start) min(e, W) / W.
 * Every operation is an fp64 operation in the order written, without contraction.  The update rounds lr_e to fp32
 * once and uses that value exactly where pinn_adam_step_dev uses its lr.
 * Limits: gamma > 0 and finite; milestones >= 0 and non-decreasing; step_size >= 1 (STEP); t_max >= 1 (COSINE);
 * warmup_epochs >= 0; 0 <= warmup_start <= 1; eta_min finite.  Fields a kind does not use are ignored. */
enum { PINN_LR_CONSTANT = 0, PINN_LR_MULTISTEP = 1, PINN_LR_STEP = 2, PINN_LR_EXPONENTIAL = 3, PINN_LR_COSINE = 4 };
#define PINN_LR_MAX_MILESTONES 16
typedef struct {
  int32_t kind;                                   /* PINN_LR_* */
  int32_t n_milestones;
  int64_t milestones[PINN_LR_MAX_MILESTONES];
  int64_t step_size, t_max, warmup_epochs;
  double gamma, eta_min, warmup_start;
} pinn_lr_schedule_t;
/* lr_e on the host, by the formula above (NaN: null or invalid schedule, or e < 0; see pinn_last_error). */
double pinn_lr_schedule_value(const pinn_lr_schedule_t* schedule, double lr0, int64_t e);

/* Squared global gradient norm: the fp64 sum of the squares of all entries of up to two fp32 vectors (g1 NULL with
 * n1 = 0: one vector) into scratch[0].  One launch: a grid-stride loop of 16-byte loads (4-byte loads of the same
 * quads where a vector is not 16-byte aligned - the grouping, and so the result, does not depend on alignment), fp64
 * accumulation, wave reduction by shuffles, per-block partials (at most 256 blocks per vector, vector 0's numbered
 * before vector 1's), and the last block to finish folds them in a fixed order: its thread t adds partials t and
 * t + 256, then a pairwise tree combines the 256 thread sums (block_fold and strided_tree_fold of
 * nsfnet_amd/csrc/fixed_fold.h, where every such order is written once).  No float atomics: the result is bit-reproducible,
 * and ranks that hold the same all-reduced gradient get the same value.  A NaN entry gives NaN.
 * scratch: pinn_grad_sqnorm_scratch_bytes() bytes of device memory, 8-byte aligned, ZERO before the first call (the
 * call leaves its workgroup ticket 0); one scratch serves one stream at a time.  As doubles: [0] the sum, [1] the
 * ticket, then block partials. */
int64_t pinn_grad_sqnorm_scratch_bytes(void);
int pinn_grad_sqnorm(const float* g0, int64_t n0, const float* g1, int64_t n1, double* scratch, void* stream);

/* pinn_adam_step_dev with the learning rate of epoch e = epoch[0] (one int64 in device memory) in place of lr, and,
 * when sqnorm is given, with every gradient entry multiplied first by the clip_grad_norm_ coefficient
 *   coef = min(1, max_norm / (sqrt(sqnorm[0]) + 1e-6))      (fp64, rounded to fp32 once; a NaN norm gives NaN)
 * in fp32, as its own rounded operation.  grads is only read.  sqnorm NULL: no clipping (max_norm is ignored, coef
 * is 1 and the gradient is used as it is); otherwise max_norm > 0.  With schedule PINN_LR_CONSTANT, no warm-up and no
 * clipping the result equals pinn_adam_step_dev's bit for bit.
 * When its last workgroup is done the call increments step_counter[0] (two int64 words as for pinn_adam_step_dev)
 * and, with advance != 0, epoch[0]; then it writes record (PINN_OPTIM_RECORD doubles, device; the caller zeroes it
 * once):
 *   [0] the epoch e used  [1] lr_e used (the fp32 value)  [2] the total norm sqrt(sqnorm[0]) (0 without clipping)
 *   [3] coef (the fp32 value)  [4] updates clipped so far (coef < 1)  [5] updates made;
 * [4] and [5] count the calls with advance != 0 only.  Several nets updated in one step must share lr_e and coef:
 * call with advance = 0 for all but the last, which advances the epoch once.  One launch. */
#define PINN_OPTIM_RECORD 6
int pinn_adam_step_sched(float* params, const float* grads, float* m, float* v, int64_t n,
                         const pinn_lr_schedule_t* schedule, double lr0, float beta1, float beta2, float eps,
                         int64_t* step_counter, int64_t* epoch, int advance, const double* sqnorm, double max_norm,
                         double* record, void* stream);

/* ---- random weight factorization of the dense layers ------------------------------------
 * Every Linear layer l = 0..L of a net (the first and the output layer included) gets its weight as
 * W_l = diag(g_l) V_l with a trainable scale factor s_l,i per ROW and g_l,i = fp32(exp((double) s_l,i)), rounded once
 * (RWF; Wang, Wang, Sankaran & Perdikaris 2022).  The factorisation is a reparametrisation between the optimizer and
 * pinn_net_prepare: no sweep, dW or prepare kernel knows about it.  With P = pinn_net_num_params and R = sum of the
 * layers' row counts = L * hidden + n_out, the trainable vector theta has P + R fp32 entries: the first P in
 * state_dict order with V_l where W_l stands (biases as they are), then the R scale factors, layers ascending and
 * rows ascending.  The optimizers (pinn_adam_step*, pinn_lbfgs_*) and pinn_grad_sqnorm take theta and its gradient
 * like any other vector of P + R entries.
 *   split    V_l[i,j] = W_l[i,j] / g_l,i (one fp32 division), b_l and s copied.  params is only read: the caller
 *            keeps using it until the first update, so turning the factorisation on changes no evaluation.
 *   compose  W_l[i,j] = g_l,i V_l[i,j] (one rounded fp32 multiply), b_l copied: params as pinn_net_prepare reads it.
 *   grad     from the effective gradient G (d loss / d params, P entries):
 *              dV[i,j] = g_i G_W[i,j] (one rounded fp32 multiply),  db = G_b,
 *              ds_i    = fp32( (double) g_i * sum_j (double) V[i,j] (double) G_W[i,j] ).
 *            The sum is fp64, not contracted, in a fixed order: one wave per row, lane t adds j = t, t + 64, ...
 *            ascending, the lanes are combined by a shuffle-down tree with offsets 32, 16, ..., 1.  No atomics, no
 *            scratch: the result is bit-reproducible.
 * One launch each.  All vectors are device memory, 4-byte aligned; an output must not overlap an input.
 * Number of scale factors R of a net (-1: null net): */
int64_t pinn_rwf_rows(pinn_net_t net);
/* theta [P + R] from params [P] and s [R]. */
int pinn_rwf_split(pinn_net_t net, const float* params, const float* s, float* theta, void* stream);
/* params [P] from theta [P + R]. */
int pinn_rwf_compose(pinn_net_t net, const float* theta, float* params, void* stream);
/* gtheta [P + R] = d loss / d theta from theta [P + R] and grads [P] = d loss / d params. */
int pinn_rwf_grad(pinn_net_t net, const float* theta, const float* grads, float* gtheta, void* stream);

/* ---- validation error on the device and the best-weights snapshot ----------------------
 * The error every training option is judged by - the relative L2 error of (u, v, p) against reference fields - as
 * device state, so that a captured step can record it at a cadence and keep the weights of its best moment without a
 * host synchronisation.  After pinn_value_forward has written the prediction planes of the n validation points,
 * per channel c in (u, v, p) over its valid points (a target that is NaN or not finite masks the point for that
 * channel, the rule of pinn_value_forward), in fp64 from the fp32 planes, one rounding per operation written except
 * that (c^ - c)^2 enters D_c by one fused multiply-add, every sum in a fixed order (no float atomics; bit-reproducible):
 *   D_c = sum (c^ - c)^2,  T_c = sum c^2,  n_c = the valid count;  for p also  A = sum d,  B = sum p,  d = p^ - p
 *   e_c  = sqrt(D_c / T_c)                                   a fraction, not percent
 *   e_p0 = sqrt(max(D_p - A^2 / n_p, 0) / (T_p - B^2 / n_p)) the pressure error up to a constant (a cavity fixes the
 *          pressure only up to one); a difference of sums: its error grows with 1 + mean(d)^2 / var(d)
 *   metric (launch constant): 0 uv = sqrt((D_u + D_v) / (T_u + T_v)), 1 e_u, 2 e_v, 3 e_p, 4 e_p0
 * A channel without valid targets gives NaN for its entries and for a metric that depends on it.
 *
 * state: PINN_VAL_STATE doubles of device memory:
 *   [0] n_records  [1] best_metric (+inf at the start)  [2] best_t  [3] stale (validations since the last
 *   improvement)  [4] nonfinite (validations whose metric was NaN or infinite)  [5] improved (0 / 1, of the last
 *   validation)  [6] cadence records so far  [7] 0.
 * The caller starts it as {0, +inf, 0, 0, 0, 0, 0, 0}.  improved is the strict metric < best_metric; a NaN or infinite
 * metric never improves.
 * ring: capacity rows of PINN_VAL_RECORD doubles; a validation writes row n_records % capacity:
 *   [0] t  [1] e_u  [2] e_v  [3] e_p  [4] e_p0  [5] metric  [6] improved  [7] n_p.
 * t = -1 (the cadence case): the row's t is (state[6] + 1) * every, read from the state, so one captured launch
 * records the right position on every replay; otherwise t (finite, >= 0) is recorded as given and state[6] stays.
 * scratch: pinn_val_scratch_bytes() bytes of device memory, 8-byte aligned, ZERO before the first call (the launch
 * leaves its workgroup ticket, the double [0], at 0); as doubles [1..11] hold the sums of the last launch:
 *   D_u T_u n_u  D_v T_v n_v  D_p T_p n_p  A  B;  then block partials.  One scratch serves one stream at a time.
 * pred3 / tgt3: host arrays of three device pointers, each plane 16-byte aligned with ceil4(n) readable floats
 * (nothing past n reaches a result); [2] of both NULL: no pressure (metrics 3 and 4 are then refused).
 * One launch: a grid-stride loop of 16-byte loads, wave reduction by shuffles, per-block partials; the last block to
 * finish folds them in block order, finishes the record and updates state and ring. */
#define PINN_VAL_RECORD 8
#define PINN_VAL_STATE 8
int64_t pinn_val_scratch_bytes(void);
int pinn_val_stats(int64_t n, const float* const* pred3, const float* const* tgt3, int metric, double t, int64_t every,
                   double* scratch, double* state, double* ring, int64_t capacity, void* stream);
/* dst0[0..n0) = src0[0..n0) and, n1 > 0, dst1[0..n1) = src1[0..n1) when state[5] (improved) is 1; nothing is written
 * when it is 0.  The condition is read from device memory, so the launch is the same every time (capturable).
 * n0 >= 1, n1 >= 0; 4-byte aligned fp32 segments.  One launch. */
int pinn_val_keep(const float* src0, float* dst0, int64_t n0, const float* src1, float* dst1, int64_t n1,
                  const double* state, void* stream);

/* ---- flow diagnostics: stream function, vorticity and vortices on the device -----------
 * Which steady solution a net is converging to, as device state: the cavity benchmark quantities of the field planes
 * a residual forward (pinn_residual_forward) left on a tensor grid of nx x ny nodes.  Node (i, j) is point j nx + i (x
 * fastest); xs [nx], ys [ny] are fp64 device arrays, strictly increasing (the plan's fp32 coordinates widened); the grid
 * need not be uniform.  fields: [PINN_FLD_COUNT][npad] floats, 16-byte aligned, npad a multiple of 4 and >= nx ny
 * (nothing past point nx ny reaches a result).  Everything is fp64 from the fp32 planes, one rounding per operation
 * written, no contraction, no float atomics; the three sums have a fixed order (block partials of a grid-stride loop of
 * min(ceil(n / 1024), 512) workgroups of 256 threads x 4 points, folded by the last workgroup: thread t takes partials
 * t, t + 256, ... in order, then a pairwise tree); an extremum does not depend on the order: on a tie the lowest
 * point wins.  3 <= nx, ny and nx ny <= 2^30, what a plan accepts.
 *
 * pinn_flow_stream_function (one launch, one thread per column, sequential in j: the trapezoid rule):
 *   psi(i, 0) = 0,  psi(i, j) = psi(i, j - 1) + (0.5 (u(i, j) + u(i, j - 1))) (ys[j] - ys[j - 1])
 * psi: nx ny doubles, 16-byte aligned.
 *
 * pinn_flow_stats (two launches) reads the planes and psi.  With w = v_x - u_y, div = u_x + v_y per node, the midlines
 * xm = (xs[0] + xs[nx - 1]) 0.5, ym likewise, and the quadrants BL (x < xm, y < ym), BR (x >= xm, y < ym), TL (x < xm,
 * y >= ym), TR, from which the lid row j = ny - 1 is left out, it writes one row of PINN_FLOW_RECORD doubles:
 *   [0] t  [1] x_c  [2] y_c  [3] psi_min  [4] w at that node          the primary vortex: argmin psi over all nodes
 *   [5 + 4q .. 8 + 4q] x, y, psi_max, area  for q = BL, BR, TL, TR     argmax psi of the quadrant; area = the quadrant's
 *                                                                     nodes with psi > eps |psi_min|, divided by nx ny
 *   [21] counter_area = ((area_BL + area_BR) + area_TL) + area_TR     [22] mass_defect = max |psi| on the lid row
 *   [23] ke = sum (u u + v v) / (nx ny)   [24] enstrophy = sum w w / (nx ny)   [25] div_rms = sqrt(sum div div / (nx ny))
 *   [26] div_max = max |div|   [27] nonfinite = the nodes where psi, w or div is not finite   [28..31] +0
 * A centre (x, y) is the node's, refined per axis by the parabola through its two neighbours on that axis:
 *   d = 0.5 (a - c) / ((a - 2 b) + c) clipped to +-0.5 (0 when the denominator is 0 or the node lies on the grid's edge of
 *   that axis);  x = xs[i] + |d| (xs[i2] - xs[i]),  i2 = i + 1 for d > 0, else i - 1, kept inside the grid.
 * nonfinite > 0: entries [1..26] are quiet NaNs - a poisoned field shows no vortex.  A quadrant without a node below the
 * lid row (possible on a coarse non-uniform grid) has NaN for x, y, psi_max and area 0.
 * state: PINN_FLOW_STATE doubles of device memory, zero at the start:
 *   [0] n_records  [1] cadence records so far  [2] records with nonfinite > 0  [3..7] 0.
 * ring: capacity rows; a call writes row n_records % capacity.  t = -1 (the cadence case): the row's t is
 * (state[1] + 1) * every, read from the state, so one captured launch records the right position on every replay;
 * otherwise t (finite, >= 0) is recorded as given and state[1] stays.  eps is finite and >= 0; the threshold
 * eps |psi_min| is formed on the device from the first launch's result.
 * scratch: pinn_flow_scratch_bytes() bytes of device memory, 8-byte aligned, ZERO before the first call (every launch
 * leaves its workgroup ticket, the double [0], at 0); as doubles [1..16] hold psi_min, its point, (psi_max, point) per
 * quadrant, the three sums, div_max, mass_defect, nonfinite of the last call, [17..20] the quadrant counts; then block
 * partials.  One scratch serves one stream at a time. */
#define PINN_FLOW_RECORD 32
#define PINN_FLOW_STATE 8
int64_t pinn_flow_scratch_bytes(void);
int pinn_flow_stream_function(int64_t nx, int64_t ny, const float* fields, int64_t npad, const double* ys, double* psi,
                              void* stream);
int pinn_flow_stats(int64_t nx, int64_t ny, const float* fields, int64_t npad, const double* xs, const double* ys,
                    const double* psi, double eps, double t, int64_t every, double* scratch, double* state, double* ring,
                    int64_t capacity, void* stream);

/* ---- hard boundary conditions: the cavity's wall values by an output transform ---------
 * The no-slip walls and the lid of the lid-driven unit cavity hold by construction instead of by a penalty term: a
 * constrained plan evaluates
 *   u = g + D N_u,   v = D N_v,   p = N_p            (N: the net's three outputs)
 * with D = 0 on the four walls and g the lid profile lifted into the cavity.  The descriptor places the unit cavity in
 * the net's input coordinates (xi, eta):  X = (xi - x0) inv_len,  Y = (eta - y0) inv_len  (plain NSFnet: x0 = y0 = 0,
 * inv_len = 1; ev-NSFnet's coordinate map: x0 = y0 = -1, inv_len = 1/2).  Derivatives in X, Y are the scaled
 * derivatives of the residual calls: a residual call on a constrained plan whose coord_scale * inv_len differs from 1
 * by more than 1e-6 is refused.
 *   D   = 16 X(1-X) Y(1-Y)      D_X = 16 (1-2X) Y(1-Y)      D_Y = 16 X(1-X) (1-2Y)      Lap D = -32 [X(1-X) + Y(1-Y)]
 *   l   = 1 - c cosh(r (X - 1/2))    l' = -r c sinh(r (X - 1/2))    l'' = -r^2 c cosh(r (X - 1/2))
 *         r = lid_sharpness,  c = 1 / cosh(r / 2) (computed in double, passed to the kernels as a float)
 *   g   = l Y^m     g_X = l' Y^m     g_Y = l m Y^(m-1)     Lap g = l'' Y^m + l m (m-1) Y^(m-2)
 *         m = lift_power, 1..8, by repeated multiplication
 * and for c in (u, v), g = 0 for v:
 *   c = g + D N     c_X = g_X + D_X N + D N_X   (Y alike)     Lap c = Lap g + Lap D N + 2 (D_X N_X + D_Y N_Y) + D Lap N
 * Residuals, field planes, loss sums and the lagged viscosity use the constrained u, v: every reader of the field
 * planes sees the physical field.  The reverse sweep starts from the transpose (a_ the adjoints of c, c_X, c_Y, Lap c):
 *   N_ = D a + D_X a_X + D_Y a_Y + Lap D a_D     N_X_ = D a_X + 2 D_X a_D     N_Y_ = D a_Y + 2 D_Y a_D     N_D_ = D a_D
 * then the scale factors; the output-bias gradient sums N_.  Value plans: pred_u = g + D N_u, pred_v = D N_v, and
 * the output adjoints the forward leaves for pinn_value_backward are coef (pred - tgt) D for u and v.  An out_adj
 * handed to pinn_value_backward is an adjoint of the NET's outputs, as on any plan.
 * By default a constrained plan runs the 8-wave kernel families (fwd / fwd_wide / fwd_bf16 / fwd_bf16_wide and their
 * reverse sweeps) whatever PINN_SCHED, PINN_WSPLIT and PINN_FUSE say.  With PINN_HBC_SPLIT=1 in the environment when
 * the plan is created it keeps the role-split, wide role-split and fused sweeps those switches give it (fwd_split /
 * bwd_split / fwdbwd_split at hidden 256, fwd_wsplit / bwd_wsplit at hidden 288 .. 448), which have constrained
 * variants too; the pipelined schedule has none, so a sweep that would run it (PINN_SCHED=1, one role-split sweep
 * without the other, an fp32 dW) runs the 8-wave kernel instead.  Forward-only calls (save = 0) and value plans run
 * the constrained 8-wave kernels either way, and an unconstrained plan never looks at the switch.  Only a net with
 * n_out = 3 can be constrained.  The constraint is a compile-time variant of those kernels: an unconstrained plan runs
 * what it ran before. */
enum { PINN_HARD_BC_NONE = 0, PINN_HARD_BC_CAVITY = 1 };
typedef struct {
  int32_t kind;        /* 0 none, 1 lid-driven unit cavity */
  int32_t lift_power;  /* m, 1..8 */
  float x0, y0, inv_len, lid_sharpness;
} pinn_hard_bc_t;
/* bc NULL or kind 0: pinn_plan_create.  Refused (pinn_last_error): n_out != 3, an unknown kind, lift_power outside
 * 1..8, a field that is not finite, inv_len <= 0, |lid_sharpness| > 150 (exp(r / 2) must stay a finite float). */
int pinn_plan_create_constrained(pinn_net_t net, int64_t n_points, int streams, const pinn_hard_bc_t* bc,
                                 pinn_plan_t* out);
/* What the plan carries (kind 0 and zeros for an unconstrained plan). */
int pinn_plan_hard_bc(pinn_plan_t plan, pinn_hard_bc_t* out);

/* ---- pseudo-time stepping of the residual loss, with device-held anchors ---------------
 * Every point of a pseudo-time plan carries an anchor (u*, v*, p*): the field at that point when the anchors were last
 * refreshed.  With the rates sigma = 1 / dtau >= 0 and sigma_p >= 0 (artificial compressibility) the residual term
 * minimises
 *   q1 = eq1 + sigma   (u - u*)
 *   q2 = eq2 + sigma   (v - v*)
 *   q3 = eq3 + sigma_p (p - p*)
 *   eq4 = eq1 (u - 1/2) + eq2 (v - 1/2) - e        (ev flavour; on the STEADY eq1, eq2, unchanged)
 *   loss_e = alpha_e / N  sum_i w_i (q1^2 + q2^2 + q3^2 + 0.1 eq4^2)
 * eq1..eq3 the steady residuals; on a constrained plan u, v are the constrained fields.  For fixed anchors this is one
 * backward-Euler step of the pseudo-transient equations; at u = u* it is the steady loss, so the steady solution is a
 * fixed point.  The reverse sweep starts from (coef_k = coef_eq4[k], q_k rebuilt from the planes and the anchors)
 *   g_k = coef_k w q_k (k = 1..3)     g4 = coef_4 w eq4
 *   r1 = g1 + g4 (u - 1/2)     r2 = g2 + g4 (v - 1/2)     r3 = g3
 *   adj(u) = r1 u_x + r2 v_x + g4 eq1 + sigma g1     adj(v) = r1 u_y + r2 v_y + g4 eq2 + sigma g2
 *   adj(p value) = sigma_p g3
 * every other output adjoint and ebar = -g4 as on any residual plan; on a constrained plan adj(u), adj(v) enter the
 * transpose with the new terms included.  The field planes keep what every reader expects: EQ1..EQ4 the steady
 * residuals, U, V, P the fields.  Loss sums 0..2 hold sum w q_k^2, slot 3 is unchanged.
 * The term is a compile-time variant of the 8-wave kernel families (fwd / fwd_wide / fwd_bf16 / fwd_bf16_wide and
 * their reverse sweeps), of the role-split sweeps (fwd_split / bwd_split / fwdbwd_split at hidden 256, fwd_wsplit /
 * bwd_wsplit at hidden 288 .. 448), with and without hard walls; the pipelined sweeps have none.  By default a
 * pseudo-time plan resolves as PINN_SCHED=0 PINN_WSPLIT=0 PINN_FUSE=0 would, whatever the environment says, and
 * pinn_plan_kernel reports the 8-wave names.  With PINN_PTIME_SPLIT=1 in the environment when the plan is created it
 * keeps the role-split, wide role-split and fused sweeps that PINN_SCHED, PINN_FWD_SCHED, PINN_BWD_SCHED, PINN_WSPLIT
 * and PINN_FUSE give a plain plan - the same names, workspace bytes and padded points - except that a sweep which would
 * run the pipelined kernels (PINN_SCHED=1, one role-split sweep without the other, an fp32 dW) runs the 8-wave kernel
 * instead; the fused kernel computes bit for bit what the two launches compute.  Forward-only calls (save = 0) run the
 * 8-wave variant either way.  A pseudo-time plan never looks at PINN_HBC_SPLIT (with walls, PINN_PTIME_SPLIT alone
 * decides), and no other plan looks at PINN_PTIME_SPLIT: any other plan runs what it ran before.
 * pinn_plan_create_pseudo_time: a residual (4-stream) plan that launches the variant; bc as for
 * pinn_plan_create_constrained (NULL or kind 0: no hard walls).
 * pinn_plan_set_pseudo_time: anchor = [3][padded] fp32 on the device (planes u*, v*, p*; padded =
 * pinn_plan_padded_points), 16-byte aligned; it stays the caller's.  The rates are launch constants of the residual
 * calls that follow.  Refused: any other plan, a negative or non-finite rate, a NULL or misaligned anchor.  A residual
 * call on a pseudo-time plan whose anchor is unset is refused (pinn_last_error).
 * pinn_plan_pseudo_time: the rates the plan carries (0, 0 until set; refused on any other plan). */
int pinn_plan_create_pseudo_time(pinn_net_t net, int64_t n_points, const pinn_hard_bc_t* bc, pinn_plan_t* out);
int pinn_plan_set_pseudo_time(pinn_plan_t plan, const float* anchor, float sigma, float sigma_p);
int pinn_plan_pseudo_time(pinn_plan_t plan, float* sigma, float* sigma_p);

/* One launch per optimiser update: the record of the pseudo-time state and, on its cadence, the anchor refresh.
 * fields = [PINN_FLD_COUNT][npad] planes of the last evaluation, anchor = [3][npad], both 16-byte aligned, npad >= n and
 * a multiple of 4; w = [n] weights, 16-byte aligned, or NULL (= 1).  With du = u - u*, dv = v - v*, dp = p - p*, each
 * in fp64 from the fp32 inputs, sums in a fixed order (no float atomics, bit-reproducible), record =
 *   [0..2] sum w eq_k^2 (the steady sums)     [3] sum w (du^2 + dv^2)     [4] sum w dp^2
 *   [5] max(|du|, |dv|), NaN-propagating      [6] updates since the last refresh, after this call     [7] refreshes made
 * When record[6] + 1 >= every (every >= 1; 0: never), or force != 0, the anchors are overwritten with the current U, V,
 * P (in whole quads of four points, up to the next multiple of 4 past n), [6] becomes 0 and [7] goes up by one;
 * otherwise [6] goes up by one.  The condition is read from device memory at kernel entry: one captured launch serves a
 * whole stage.  record: PINN_PTIME_RECORD doubles of device memory, zero before the first call, 8-byte aligned.
 * scratch: pinn_ptime_scratch_bytes(n) bytes of device memory, 8-byte aligned, ZERO before the first call (the launch
 * leaves its ticket word 0 again); -1 for n outside 1..2^30. */
#define PINN_PTIME_RECORD 8
int64_t pinn_ptime_scratch_bytes(int64_t n);
int pinn_ptime_advance(int64_t n, const float* fields, int64_t npad, const float* w, float* anchor, int64_t every,
                       int force, double* scratch, double* record, void* stream);

/* ---- convergence monitor: a stage that has stopped making progress is noticed on the device ----
 * Two launches, both meant for the captured step; the host reads the state at its log points only.
 * pinn_monitor_vis_stats: over vis_t = [n] fp32 (non-negative entries, 16-byte aligned; the last quad is read by
 *   element), in fp64 with a fixed order (no float atomics, bit-reproducible): the sum, rounded once to fp32, into
 *   *sum_out - a free slot of the loss-sum block, so that the exchange that is made anyway turns it into the global sum -
 *   and, for this rank alone, info (PINN_MON_INFO doubles) =
 *     [0] max entry, NaN-propagating     [1] entries >= vis_t0 (compared in fp32)     [2] the fp64 sum     [3] n
 *   scratch: pinn_monitor_scratch_bytes() bytes of device memory, 8-byte aligned, ZERO before the first call (the launch
 *   leaves its ticket word 0 again).
 * pinn_monitor_observe: one workgroup, after an optimiser update.  eq, bc, sup: the three loss-sum blocks (PINN_NLOSS
 *   floats each; sup NULL: no supervised term) of the evaluation that produced the update, after the exchange - eq[4] is
 *   the slot pinn_monitor_vis_stats wrote.  lam: the balancing weights (lambda_b, lambda_s) in device memory, or NULL:
 *   the launch constants alpha_b, alpha_s.  state[0] goes up by one (t); unless t % every == 0 nothing else happens.
 *   An observation, every operation fp64 from the fp32 sums, rounded once, in this order:
 *     eq_k = eq[k] / n_eq (k = 0..3)       loss_e = (eq_0 + eq_1) + eq_2       ev:  loss_e = loss_e + eq4_weight eq_3
 *     loss_b = (bc[0] + bc[1]) / n_b       loss_s = (sup[0] + sup[1]) / n_s  [ + sup[2] / n_p  where n_p > 0 ]   (n_s = 0: 0)
 *     loss = ((w_b loss_b) + (alpha_e loss_e)) + (w_s loss_s)
 *     vis_mean = eq[4] / n_eq (ev; else 0)       Re_eff = 1 / (1 / Re + vis_mean)
 *   the row (PINN_MON_RECORD doubles), written at ring[(observations so far) % capacity]:
 *     [0] t
 *     [1] loss
 *     [2] loss_e
 *     [3] loss_b
 *     [4] loss_s
 *     [5..8] eq_0 .. eq_3
 *     [9] vis_mean
 *     [10] Re_eff
 *     [11] the stop code after this observation
 *   A non-finite loss is counted, sets PINN_MON_STOP_NONFINITE and stays out of the window.  Otherwise Q (quantity: 0
 *   loss, 1 loss_e, 2 loss_b) and Re_eff join the window sums; at `window` observations the window means (sum / window)
 *   are compared with the previous window's (the first complete window only sets them) and the window restarts:
 *     plateau_on:  prev == 0 or (prev - mean) / |prev| < min_rel_improvement  ->  stale + 1, else stale = 0
 *     re_eff_on:   |mean_re - prev_re| / prev_re < re_eff_tol                 ->  settled + 1, else settled = 0
 *   At every observation with t >= min_updates: stale >= patience sets PINN_MON_STOP_PLATEAU, settled >= patience sets
 *   PINN_MON_STOP_RE_EFF.  The bits are sticky; the call sets bits and writes nothing else.
 *   state (PINN_MON_STATE doubles of device memory, zero at the start, 8-byte aligned):
 *     [0] updates counted (t)
 *     [1] observations (rows written)
 *     [2] observations with a non-finite loss
 *     [3] observations in the current window
 *     [4] sum of Q over the current window
 *     [5] sum of Re_eff over the current window
 *     [6] complete windows
 *     [7] mean of Q over the last complete window
 *     [8] mean of Re_eff over the last complete window
 *     [9] stale
 *     [10] settled
 *     [11] stop code (PINN_MON_STOP_* bits)
 *     [12] t of the observation that set PLATEAU (0: not set)
 *     [13] t of the observation that set RE_EFF
 *     [14] t of the observation that set NONFINITE
 *     [15] 0
 *   Refused with -22 (pinn_last_error names the field): every < 1, window < 1, patience < 1, capacity < 1,
 *   min_updates < 0, a quantity outside 0..2, a tolerance that is switched on and negative or not finite, re_eff_on
 *   without ev; n_eq or n_b < 1, n_s or n_p < 0, Re not finite and > 0. */
#define PINN_MON_RECORD 12
#define PINN_MON_STATE 16
#define PINN_MON_INFO 4
enum { PINN_MON_STOP_PLATEAU = 1, PINN_MON_STOP_RE_EFF = 2, PINN_MON_STOP_NONFINITE = 4 };
typedef struct {
  int64_t every, window, patience, min_updates, capacity;
  int32_t quantity;     /* 0 loss, 1 loss_e, 2 loss_b */
  int32_t ev;           /* != 0: the ev flavour - eq4 enters loss_e, eq[4] holds the vis_t sum */
  int32_t plateau_on, re_eff_on;
  double min_rel_improvement, re_eff_tol;
} pinn_monitor_config_t;
int64_t pinn_monitor_scratch_bytes(void);
int pinn_monitor_vis_stats(int64_t n, const float* vis_t, float vis_t0, float* sum_out, double* info, double* scratch,
                           void* stream);
int pinn_monitor_observe(const float* eq, const float* bc, const float* sup, const float* lam, double alpha_b,
                         double alpha_s, double alpha_e, double eq4_weight, double n_eq, double n_b, double n_s, double n_p,
                         double Re, const pinn_monitor_config_t* cfg, double* state, double* ring, void* stream);

/* ---- viscosity identification: the molecular viscosity nu = 1 / Re as a trainable scalar ----
 * pinn_plan_set_viscosity: a residual (4-stream) plan may carry two device pointers.  nu_dev: one fp32; every residual
 *   launch of the plan (forward, reverse sweep, fused) then uses *nu_dev wherever it would use 1 / Re - the Re argument of
 *   those calls is still checked and otherwise unused.  lap: [2][padded points] fp32, 16-byte aligned; the forward leaves
 *   the physical Laplacians Lap u, Lap v there (after coord_scale^2; on a constrained plan those of the constrained
 *   fields), padded like the field planes.  lap may be NULL (a plan that is only evaluated); nu_dev = NULL with lap = NULL
 *   turns both off, and the plan computes what it computed before the call, bit for bit.  A value-mode plan, lap
 *   without nu_dev and misaligned pointers are refused with -22.  pinn_plan_viscosity returns the two pointers.
 * pinn_visc_grad: one streaming launch over the planes an evaluation left.  Per point i < n, fp64 from the fp32
 *   planes, one rounding per operation in this order:
 *     a1 = eq1 + (w4 eq4) (u - 1/2)     a2 = eq2 + (w4 eq4) (v - 1/2)     t_i = w_i ((a1 Lap u) + (a2 Lap v))
 *   (w NULL: w_i = 1; w4 = 0: a1 = eq1, a2 = eq2 and the eq4, u, v planes are not read).  S = sum t_i in a fixed order (no
 *   float atomics, bit-reproducible), rounded once to fp32 into *sum_out - a free slot of the loss-sum block, so that
 *   the exchange that is made anyway turns it into the global sum.  d loss / d nu = -(2 alpha_e / N) S.
 *   fields, lap, w 16-byte aligned, npad % 4 == 0.  scratch: pinn_visc_scratch_bytes(n) bytes of device memory, 8-byte
 *   aligned, ZERO before the first call (the launch leaves its ticket word 0 again).
 * pinn_visc_update: one workgroup, after the nets' updates.  s = (double)*sum.  A non-finite s raises state[7] and
 *   changes nothing else.  Otherwise, fp64, one rounding per operation in this order (torch.optim.Adam on theta = ln nu):
 *     G = coef s                 g = (double)*nu_dev G
 *     p1 = state[3] beta1        p2 = state[4] beta2
 *     m = (beta1 m) + ((1 - beta1) g)            v = (beta2 v) + (((1 - beta2) g) g)
 *     theta = theta - (lr / (1 - p1)) (m / ((sqrt(v) / sqrt(1 - p2)) + eps))
 *     theta = min(max(theta, theta_min), theta_max)          *nu_dev = (float)exp(theta)
 *   state (PINN_VISC_STATE doubles of device memory, 8-byte aligned; start: theta, 0, 0, 1, 1, 0, 0, 0):
 *     [0] theta   [1] m   [2] v   [3] beta1^t   [4] beta2^t   [5] t (updates made)   [6] the last G   [7] skipped updates */
#define PINN_VISC_STATE 8
int pinn_plan_set_viscosity(pinn_plan_t plan, const float* nu_dev, float* lap);
int pinn_plan_viscosity(pinn_plan_t plan, const float** nu_dev, float** lap);
int64_t pinn_visc_scratch_bytes(int64_t n);
int pinn_visc_grad(int64_t n, const float* fields, int64_t npad, const float* lap, const float* w, double w4,
                   float* sum_out, double* scratch, void* stream);
int pinn_visc_update(const float* sum, double coef, double lr, double beta1, double beta2, double eps, double theta_min,
                     double theta_max, double* state, float* nu_dev, void* stream);

/* ---- Reynolds-number continuation: a device-held ramp of the viscosity nu = 1 / Re (and of the cap vis_t0) ----
 * pinn_plan_set_viscosity_cap: beside nu_dev a residual plan may carry cap_dev, one fp32 of device memory; the forward
 *   launches (the fused one included) then use *cap_dev wherever they would use the vis_t0 argument, which is still
 *   checked and otherwise unused.  Refused with -22: a value-mode plan, a cap on a plan without nu_dev, a misaligned
 *   pointer.  pinn_plan_set_viscosity drops the cap (set nu_dev first, the cap second); NULL takes it off.
 *   pinn_plan_viscosity_cap returns the pointer.
 * The schedule: with t updates made so far,
 *     s = min(max((t - hold) / updates, 0), 1)        stairs = K > 0 and s < 1:  s = floor(s K) / K
 *   s <= 0 selects nu_start, cap_start and s >= 1 nu_end, cap_end: the fp32 values given, never computed, so that a
 *   finished ramp leaves the bits the launches would take as constants.  In between, fp64, one rounding per operation
 *   in the order written, with n0 = (double)nu_start, n1 = (double)nu_end:
 *     PINN_RAMP_GEOMETRIC   nu64 = exp(log(n0) + s (log(n1) - log(n0)))
 *     PINN_RAMP_LINEAR_RE   nu64 = 1 / ((1 / n0) + s ((1 / n1) - (1 / n0)))
 *     PINN_RAMP_LINEAR_NU   nu64 = n0 + s (n1 - n0)
 *   nu64 is clamped to the interval of n0 and n1, cap64 = cap_factor nu64 to that of cap_start and cap_end; nu =
 *   (float)nu64, cap = (float)cap64, Re_t = 1 / nu64 (at the ends: re_start, re_end).  Monotone in t.
 * pinn_visc_schedule_value: host only, the same function the kernel runs; record6 (may be NULL) receives the record
 *   below for position t; returns nu_t (NaN and pinn_last_error for a bad schedule or t < 0).
 * pinn_visc_schedule_step: one workgroup, after the nets' updates.  t = *pos + 1 is stored to *pos (int64: positions
 *   beyond 2^31 work), *nu_dev and (not NULL) *cap_dev are rewritten for t, and record (PINN_RAMP_RECORD doubles, 8-byte
 *   aligned) becomes [0] t  [1] s  [2] Re_t  [3] nu_t  [4] cap_t (0 without cap_factor)  [5] done (s >= 1).
 *   No atomics, bit-reproducible.  Refused with -22: updates <= 0, hold < 0, stairs < 0, an unknown shape, re_start /
 *   re_end / the fp32 ends not finite and > 0, cap_factor not finite or < 0, NULL or misaligned pointers. */
#define PINN_RAMP_RECORD 6
enum { PINN_RAMP_GEOMETRIC = 0, PINN_RAMP_LINEAR_RE = 1, PINN_RAMP_LINEAR_NU = 2 };
typedef struct {
  int32_t shape;                /* PINN_RAMP_* */
  int32_t stairs;               /* K: the ramp in K equal stairs; 0: smooth */
  int64_t hold, updates;        /* updates at the start value before the ramp; its length */
  double re_start, re_end;      /* the Reynolds numbers of the ends (the record's Re_t there) */
  double cap_factor;            /* vis_t0_factor: cap = cap_factor nu inside the ramp; 0: no cap */
  float nu_start, nu_end;       /* the fp32 written at s <= 0, at s >= 1 */
  float cap_start, cap_end;
} pinn_visc_schedule_t;
int pinn_plan_set_viscosity_cap(pinn_plan_t plan, const float* cap_dev);
int pinn_plan_viscosity_cap(pinn_plan_t plan, const float** cap_dev);
double pinn_visc_schedule_value(const pinn_visc_schedule_t* schedule, int64_t t, double* record6);
int pinn_visc_schedule_step(const pinn_visc_schedule_t* schedule, int64_t* pos, float* nu_dev, float* cap_dev,
                            double* record, void* stream);

/* ---- training-state snapshots: many device buffers <-> one staging buffer, with digests ----
 * A snapshot is a list of segments (any number; a launch takes up to 64, more take several launches).  In the staging
 * buffer segment k starts at align256(end of the segment stored before it) and the padding behind a segment is zero,
 * so two snapshots of one state are the same bytes.  Every segment size is a multiple of 4 (others are refused).
 * The digest of a segment reads its bytes as little-endian 32-bit words w_0 .. w_{n-1}:
 *   A = sum w_i mod 2^64      B = sum (i + 1) w_i mod 2^64
 * - modular integer sums, independent of order and grid.  float32 [1..8] gives (8648654848, 39057358848).
 * pinn_state_layout: host only; offsets_out[k] for the sizes bytes[k] (a segment that is not stored is given size 0
 *   here), returns the total size, -1 on a bad size.
 * pinn_state_digest_host: host only; the digest of host memory into out2 = (A, B) - what verifies a file before
 *   anything is uploaded.
 * pinn_state_pack: copies the device buffers src[k] (bytes[k] each, 4-byte aligned) to dst + offsets[k], zeroes the
 *   padding behind each (up to the next multiple of 256 or the end of dst) and writes the digests (A, B) of segment k to digests_out[2 k], [2 k + 1] (device memory).
 *   offsets[k] = -1: digest only - src[k] is read and digested, nothing is stored.  The offsets must ascend, be multiples
 *   of 256 and stay inside dst_bytes (all checked before anything is launched); dst 16-byte aligned.
 * pinn_state_unpack: the reverse scatter from src + offsets[k] into the live buffers dst[k]; the digests are those of
 *   what it wrote.  offsets[k] = -1: dst[k] is digested as it stands, nothing is written.
 * Accesses are 16 bytes wide where both pointers of a segment are 16-byte aligned, 4 bytes otherwise.
 * scratch: pinn_state_scratch_bytes() bytes of device memory, 8-byte aligned, ZERO before the first call (a launch
 * leaves its ticket word 0 again); calls that share it must be ordered on one stream. */
int64_t pinn_state_scratch_bytes(void);
int64_t pinn_state_layout(int nseg, const int64_t* bytes, int64_t* offsets_out);
int pinn_state_digest_host(const void* ptr, int64_t bytes, uint64_t* out2);
int pinn_state_pack(int nseg, const void* const* src, const int64_t* bytes, const int64_t* offsets, void* dst, int64_t dst_bytes,
                    uint64_t* digests_out, void* scratch, void* stream);
int pinn_state_unpack(int nseg, const void* src, int64_t src_bytes, const int64_t* bytes, const int64_t* offsets, void* const* dst,
                      uint64_t* digests_out, void* scratch, void* stream);

#ifdef __cplusplus
}
#endif
#endif
