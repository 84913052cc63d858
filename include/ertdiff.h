/*
 * ertdiff.h -- C ABI of libertdiff_hip.so, the MI355X (gfx950) implementation
 * of the conditional-DDPM denoising hot path of pnnl/ERT-Conditional-Diffusion-Model.
 *
 * The reference has no native code and no FFI: its hot path is the Python call
 * surface in ERT_Conditional_Diffusion.py.  Each entry point below replaces the
 * ATen work behind one of those Python functions; the Python drop-in module
 * (ert-conditional-diffusion-model_amd/ertdiff) binds them with ctypes, see
 * INTEGRATION.md.
 *
 * Conventions (all entry points):
 *   - every pointer is DEVICE memory owned by the caller (torch tensors);
 *     the library never allocates or frees device memory on these paths and
 *     keeps no global state besides cached kernel handles;
 *   - float tensors are fp32, row-major contiguous; timesteps are int64;
 *   - work is enqueued on `stream` (a hipStream_t passed as void*) with no
 *     host synchronisation, so calls may be captured into a hipGraph;
 *   - return 0 on success, a negative ERTD_E* code for bad arguments (checked
 *     on the host BEFORE anything is launched), or a positive hipError_t.
 *
 * Workspace contract (every entry that takes `ws, ws_bytes`, and every output;
 * tests/test_gpu_dirty_entries.py and test_gpu_dirty_api.py enforce it on
 * 0xFF-filled, exactly sized, fenced memory):
 *   - the contents of ws and of every output on entry are ARBITRARY: no entry
 *     relies on zeros, and nothing is read before the same call has written
 *     it (counters, ring / claim / progress words, partial-sum buffers, pad
 *     lanes of packed weights and of the bf16 image are all written first);
 *   - nothing outside [ws, ws + ws_bytes) and outside the outputs is written,
 *     and nothing outside the inputs as described is read; ws_bytes equal to
 *     the entry's *_ws_bytes / *_workspace_bytes query is enough, one byte
 *     less is ERTD_ENOSPC with nothing launched and no output touched;
 *   - results do not depend on what ws held: a call on a workspace another
 *     call (another geometry, another entry) has used gives the same bits.
 * The ONLY state carried from one call to the next:
 *   - the packing at the head of ws that ertd_conv2d / ertd_conv_input_grad
 *     (or ertd_conv_pack_batch) leave for the *_run entries;
 *   - the activations ertd_train_forward / ertd_encoder_train_fwd save in ws
 *     for the matching backward;
 *   - a plan's workspace and bound buffers between its launches (head graph
 *     -> step graphs; a plan never shares ws with another stream's work);
 *   - the sampler status word (ertd_sample_status), which EVERY ertd_sample /
 *     ertd_sample_conditions / ertd_sample_solver call clears or sets, the
 *     hoisted mode included.
 *
 * Shapes: B = batch (members), L = measurements per survey (4693 in the
 * reference), C_in = 14 surveys, P = param_dim (29 in the reference, 1..32
 * supported), H = hidden_dim (128; the only value the reference uses).
 */
#ifndef ERTDIFF_H
#define ERTDIFF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ERTD_OK 0
#define ERTD_EINVAL (-1)   /* bad shape / null pointer / unsupported dim */
#define ERTD_ENOSPC (-2)   /* workspace too small */
#define ERTD_ENOGPU (-3)   /* no gfx950 device / kernel image unavailable */
#define ERTD_ETIMEOUT (-4) /* a persistent sampler wait timed out (see ertd_sample_status) */

#define ERTD_CIN 14
#define ERTD_HIDDEN 128
#define ERTD_PMAX 32

/* Pointers to the 12 state_dict tensors of ConditionalDiffusionModel
 * (ERT_Conditional_Diffusion.py:133-153), in state_dict order.          */
typedef struct ertd_weights {
  const float* enc0_w; /* condition_encoder.0.weight (32,14,3)   */
  const float* enc0_b; /* condition_encoder.0.bias   (32)        */
  const float* enc2_w; /* condition_encoder.2.weight (64,32,3)   */
  const float* enc2_b; /* condition_encoder.2.bias   (64)        */
  const float* enc6_w; /* condition_encoder.6.weight (128,64)    */
  const float* enc6_b; /* condition_encoder.6.bias   (128)       */
  const float* time_w; /* time_embed.0.weight        (128,128)   */
  const float* time_b; /* time_embed.0.bias          (128)       */
  const float* mlp0_w; /* mlp.0.weight               (128,P+256) */
  const float* mlp0_b; /* mlp.0.bias                 (128)       */
  const float* mlp2_w; /* mlp.2.weight               (P,128)     */
  const float* mlp2_b; /* mlp.2.bias                 (P)         */
  int param_dim;       /* P */
  int hidden_dim;      /* H, must be 128 */
} ertd_weights;

/* Workspace ops for ertd_workspace_bytes(). */
#define ERTD_OP_FORWARD 0
#define ERTD_OP_SAMPLE 1
#define ERTD_OP_TRAIN 2

/* Sampler modes. */
#define ERTD_MODE_HOISTED 0  /* condition encoder once, persistent T-loop   */
#define ERTD_MODE_FAITHFUL 1 /* encoder re-evaluated every step (reference):
                                one persistent launch per chain when the grid
                                fits, else the per-step schedule            */
#define ERTD_MODE_FAITHFUL_STEPS 2 /* faithful, forced per-step schedule:
                                      encoder + head launch per step        */

/* Encoder operand precision. */
#define ERTD_PREC_FP32 0
#define ERTD_PREC_BF16 1 /* bf16 conv operands, fp32 accumulate/state */
/* U-Net only: split-bf16 conv operands -- x = hi + lo (two bf16 RNE planes),
   products lo*hi + hi*lo + hi*hi on the bf16 MFMA, fp32 accumulate/state
   (about 2^-16 relative per product: within the north star's 1e-4) */
#define ERTD_PREC_BF16X3 2

int ertd_version(void);
const char* ertd_error_string(int code);
/* 1 when a gfx950 device is visible and the kernels load, else 0. */
int ertd_device_ok(void);

/* Bytes of caller-provided device workspace an op needs.
 * T = number of sampler steps (ignored for FORWARD).                      */
size_t ertd_workspace_bytes(int B, int L, int P, int T, int op);
/* Floats of packed (MFMA fragment-order) encoder weights. */
size_t ertd_packed_floats(void);

/* Re-lay the two Conv1d weights into MFMA fragment order (once per weight
 * update).  packed: ertd_packed_floats() floats.                          */
int ertd_pack_weights(const ertd_weights* w, float* packed, void* stream);

/* get_timestep_embedding (ERT_Conditional_Diffusion.py:80-88) on device.
 * freq: (dim/2) float32 frequencies exp(-i*ln(1e4)/(dim/2-1)) computed on the
 * host with the reference's float32 expression; out: (B, dim).            */
int ertd_timestep_embedding(const int64_t* t, int B, int dim, const float* freq,
                            float* out, void* stream);

/* q_sample (ERT_Conditional_Diffusion.py:96-99): out = sqrt(ab[t])*x0 + sqrt(1-ab[t])*noise. */
int ertd_q_sample(const float* x0, const int64_t* t, const float* noise,
                  const float* alpha_bar, int B, int P, float* out, void* stream);

/* condition_encoder (ERT_Conditional_Diffusion.py:133-142): cond (B,14,L) ->
 * cond_emb (B,128).                                                       */
int ertd_encoder_fwd(const ertd_weights* w, const float* packed, const float* cond,
                     int B, int L, int precision, float* cond_emb,
                     void* ws, size_t ws_bytes, void* stream);

/* The encoder's strip kernel alone (conv1 -> ReLU -> conv2 -> ReLU -> per-strip
 * pool sums), writing partial (B, n_strips, 64) into ws.  This is the hot
 * kernel of every step; exposed so callers can time it in isolation.      */
int ertd_encoder_strips(const ertd_weights* w, const float* packed, const float* cond,
                        long long cond_stride, int B, int L, int precision,
                        void* ws, size_t ws_bytes, void* stream);

/* ConditionalDiffusionModel.forward (ERT_Conditional_Diffusion.py:155-164):
 * x (B,P), t (B,) int64, cond (B,14,L) -> out (B,P).  freq as above (H/2).
 * cond_emb_out / t_emb_out: optional (B,128) intermediates (NULL to skip). */
int ertd_forward(const ertd_weights* w, const float* packed, const float* x,
                 const int64_t* t, const float* cond, int B, int L, const float* freq,
                 int precision, float* out, float* cond_emb_out, float* t_emb_out,
                 void* ws, size_t ws_bytes, void* stream);

/* sample_model's reverse loop (ERT_Conditional_Diffusion.py:107-119).
 *   cond (B,14,L) with member stride cond_stride floats (14*L when each
 *     member has its own condition, 0 when all members share one).
 *   num_steps: schedule length n of the call (reference: num_steps or T).
 *   Runs steps t = t_first, t_first-1, ..., t_first-n_run+1 (reference:
 *     t_first = n-1, n_run = n); x_inout (B,P) carries the state in/out, so a
 *     chain may be split into segments.
 *   c1, c2, sigma: (num_steps) float32 per-step scalars, index t, formed on
 *     the host with the reference's expressions (:111-118; sigma already
 *     multiplied by temperature).
 *   noise: NULL -> counter-based Philox keyed by (seed, member_offset+b, t);
 *     else (num_steps, B, P) injected draws in reference order: noise[k] is
 *     the z used at t = num_steps-k (noise[0] = x_T is not read).
 *   mode: ERTD_MODE_HOISTED / ERTD_MODE_FAITHFUL / ERTD_MODE_FAITHFUL_STEPS
 *     (bit-identical outputs).                                            */
int ertd_sample(const ertd_weights* w, const float* packed, const float* cond,
                long long cond_stride, int B, int L, int num_steps, int t_first, int n_run,
                const float* c1, const float* c2, const float* sigma, const float* freq,
                const float* noise, uint64_t seed, uint32_t member_offset, int mode,
                int precision, float* x_inout, void* ws, size_t ws_bytes, void* stream);

/* Few-step sampling on a timestep subset (DDIM, DPM-Solver++(2M)).  For K
 * descending timesteps tau_0 > ... > tau_{K-1} >= 0 step k is
 *     eps = model(x, tau_k, cond)
 *     D   = p_k x + q_k eps;  D = clamp(D, -clip, clip) when clip > 0
 *     x   = a_k x + b_k D + c_k D_prev + s_k z;   D_prev = D
 * with D_prev = 0 before step 0.  A term whose coefficient is zero is
 * skipped: D_prev is not read when c_k == 0, z is neither read nor drawn
 * when s_k == 0.
 *   timesteps (K) int32 and coef (K,6) float32, row k = {p,q,a,b,c,s}: DEVICE
 *     tables (ertdiff.schedule.solver_tables builds them).  They are read back
 *     once, blocking, on `stream` and refused with ERTD_EINVAL unless the
 *     timesteps are strictly descending and >= 0, c_0 == 0, every c_k == 0
 *     when d_prev_inout is NULL, and s_{K-1} == 0 when `noise` is given --
 *     so the call cannot be captured into a graph.
 *   Runs steps k = k_first .. k_first+n_run-1.  x_inout (B,P) and
 *     d_prev_inout (B,P, may be NULL when every c_k == 0) carry the state, so
 *     a chain split into segments equals the unsplit chain bit for bit
 *     (d_prev_inout is read only when k_first > 0).
 *   noise: NULL -> Philox keyed by (seed, member_offset+b, tau_k), the
 *     ancestral sampler's stream; else (K, B, P): noise[0] = x_T is not read,
 *     step k reads noise[k+1], the last step reads none.
 *   mode: ERTD_MODE_HOISTED only (one persistent kernel, x and D_prev in
 *     registers).  The faithful modes exist to mirror the reference's
 *     per-step encoder recompute and would give the same bits: ERTD_EINVAL.
 *   ws: ertd_workspace_bytes(B, L, P, K, ERTD_OP_SAMPLE).                  */
int ertd_sample_solver(const ertd_weights* w, const float* packed, const float* cond,
                       long long cond_stride, int B, int L, int K, int k_first, int n_run,
                       const int32_t* timesteps, const float* coef, float clip, const float* freq,
                       const float* noise, uint64_t seed, uint32_t member_offset, int mode,
                       int precision, float* x_inout, float* d_prev_inout, void* ws,
                       size_t ws_bytes, void* stream);
/* The bare update of one step on (B,P) device arrays: coef_row = 6 device
 * floats {p,q,a,b,c,s}.  x in/out; d_prev in/out (may be NULL: treated as
 * zero, D not stored); z may be NULL (treated as zero).  d_prev is read only
 * when c != 0, z only when s != 0.                                          */
int ertd_solver_update(float* x, const float* eps, float* d_prev, const float* coef_row, float clip,
                       const float* z, int B, int P, void* stream);

/* Status word of the last persistent faithful chain run on `ws` (same B, L,
 * num_steps as the ertd_sample call): synchronizes `stream`; *status = 0 and
 * ERTD_OK, or the code of the wait that timed out and ERTD_ETIMEOUT (the
 * launch then drained without finishing; x_inout is not valid).           */
int ertd_sample_status(const void* ws, int B, int L, int num_steps, int* status, void* stream);

/* Standard normals from the sampler's Philox stream: out (B,P) for members
 * member_offset..+B-1 at step `t`, stream tag `tag` (0 = step noise z_t,
 * 1 = initial x_T).                                                       */
int ertd_philox_normal(uint64_t seed, uint32_t member_offset, int B, int P, int t,
                       int tag, float* out, void* stream);

/* Ensemble post-processing (ERT_Conditional_Diffusion.py:400-406, :1054-1060):
 * u (rows, P) unconstrained samples (sample_model output) ->
 *   out (rows, P) = param_scaler.inverse_transform(inverse_transform(u, a, b))
 *     (sigmoid in float32; then MinMaxScaler's float64 min_/scale_ applied as
 *      x -= min_; x /= scale_ on the float32 array, each op rounded to float32)
 *   valid (rows) uint8 = 1 unless check_param_bounds (:183-218) rejects the row
 *     (any value < limits[p][0] or > limits[p][1], compared in float64).
 * min_, scale_: (P) float64 (a fitted MinMaxScaler's min_ and scale_);
 * limits: (P, 2) float64 [min, max] (Generate_ERT_utils.ParameterLimits.plims). */
int ertd_postprocess(const float* u, long long rows, int P, double a, double b,
                     const double* min_, const double* scale_, const double* limits, float* out,
                     uint8_t* valid, void* stream);

/* hipGraph plans: capture one full ertd_sample call (all kernels of all
 * steps) once, replay with ertd_plan_launch.  Buffers are bound at creation. */
typedef struct ertd_plan ertd_plan;
int ertd_sample_plan_create(const ertd_weights* w, const float* packed, const float* cond,
                            long long cond_stride, int B, int L, int num_steps, int t_first,
                            int n_run, const float* c1, const float* c2, const float* sigma,
                            const float* freq, const float* noise, uint64_t seed,
                            uint32_t member_offset, int mode, int precision, float* x_inout,
                            void* ws, size_t ws_bytes, ertd_plan** plan);
int ertd_plan_launch(ertd_plan* plan, void* stream);
int ertd_plan_destroy(ertd_plan* plan);

/* The reference's test-set uncertainty evaluation (ERT_Conditional_Diffusion.py
 * :1042-1069: every test condition x `uncertainty_samples` calls of
 * sample_model) as ONE sampler launch of B = n_cond * n_samples members.
 *   cond (n_cond, 14, L) contiguous; member j = realisation r = j / n_cond of
 *     condition c = j % n_cond, so x_inout (B, P) is the (n_samples, n_cond, P)
 *     `Uncertainty_params` layout (:1073) as it fills.
 *   Philox id of member j: member_offset + r * id_period + c.  One device:
 *     id_period = n_cond, member_offset = 0 (ids 0..B-1, realisation r's
 *     members r*N .. r*N+N-1: the same draws as sample_model with
 *     member_offset = r*N).  A rank holding conditions [c0, c0+n_cond) of N
 *     passes member_offset = c0, id_period = N: every member keeps its global
 *     id, so the result is bitwise invariant to how the conditions are split.
 *   ERTD_MODE_HOISTED runs the condition encoder once per CONDITION (n_cond
 *     strip sets, not B); the faithful modes re-run it per member and step as
 *     the reference does.  Workspace: ertd_workspace_bytes(B, L, P, num_steps,
 *     ERTD_OP_SAMPLE).  Other arguments as ertd_sample.                      */
int ertd_sample_conditions(const ertd_weights* w, const float* packed, const float* cond, int n_cond,
                           int n_samples, long long id_period, int L, int num_steps, int t_first,
                           int n_run, const float* c1, const float* c2, const float* sigma,
                           const float* freq, const float* noise, uint64_t seed,
                           uint32_t member_offset, int mode, int precision, float* x_inout, void* ws,
                           size_t ws_bytes, void* stream);
int ertd_sample_conditions_plan_create(const ertd_weights* w, const float* packed, const float* cond,
                                       int n_cond, int n_samples, long long id_period, int L,
                                       int num_steps, int t_first, int n_run, const float* c1,
                                       const float* c2, const float* sigma, const float* freq,
                                       const float* noise, uint64_t seed, uint32_t member_offset,
                                       int mode, int precision, float* x_inout, void* ws,
                                       size_t ws_bytes, ertd_plan** plan);

/* ---- training (ERT_Conditional_Diffusion.py:305-320) ---------------------------
 * Workspace: ertd_workspace_bytes(B, L, P, 0, ERTD_OP_TRAIN).  The forward
 * stores the activations the backward reads there: keep it between the two.
 * grads / exp_avg / exp_avg_sq: 12 device buffers in state_dict order with the
 * parameters' shapes.  The parameters are the (mutable) pointers of `w`.    */

/* Training forward: eps = model(x, t, cond) with activations saved in ws.
 * x (B,P), or x == NULL and x0/noise/alpha_bar given: x = q_sample(x0, t, noise)
 * (:314).  The train kernels read the parameters of `w` in place: `packed` is
 * unused (kept for ABI compatibility; may be NULL), here and below.          */
int ertd_train_forward(const ertd_weights* w, float* packed, const float* x, const float* x0,
                       const float* noise, const float* alpha_bar, const int64_t* t,
                       const float* cond, int B, int L, const float* freq, float* eps_out,
                       void* ws, size_t ws_bytes, void* stream);

/* Backward of the last ertd_train_forward on `ws`.  dout (B,P) = dL/deps, or
 * NULL with `noise`: L = MSELoss(mean)(eps, noise) (:295, :316), loss_out (1).
 * dx_out (B,P) optional.  grads are overwritten (not accumulated).          */
int ertd_train_backward(const ertd_weights* w, const float* packed, const float* dout,
                        const float* noise, const float* cond, int B, int L, float* const* grads,
                        float* loss_out, float* dx_out, void* ws, size_t ws_bytes, void* stream);

/* torch.optim.Adam step (no weight decay / amsgrad) on the 12 parameters of w,
 * in place.  step = the step count after this update (>= 1).               */
int ertd_adam(const ertd_weights* w, float* const* grads, float* const* exp_avg,
              float* const* exp_avg_sq, int step, float lr, float beta1, float beta2, float eps,
              void* stream);

/* The reference train step (:309-319) in one call: q_sample -> forward ->
 * MSELoss -> backward -> Adam.  loss_out (1) float32 on device; grads receive
 * the gradients (the reference's p.grad after loss.backward()).            */
int ertd_train_step(const ertd_weights* w, float* packed, const float* x0, const int64_t* t,
                    const float* noise, const float* cond, const float* alpha_bar, int B, int L,
                    const float* freq, float* const* grads, float* const* exp_avg,
                    float* const* exp_avg_sq, int step, float lr, float beta1, float beta2,
                    float eps, float* loss_out, void* ws, size_t ws_bytes, void* stream);

/* ertd_train_step with no host scalars, for graph capture (ertdiff.TrainPlan):
 * the step advances the device counter *step_dev (int32; the count of Adam
 * steps applied, as torch's state["step"]) and the update of step s uses the
 * 6-float entry adam_table[s - table_first] (device copy of ertd_adam_table's
 * output); s must lie in [table_first, table_first + table_len).  The device
 * cannot report a step outside the table: it CLAMPS s to the nearest entry
 * (wrong bias corrections, no error), so the caller re-builds the table before
 * it runs out (ertdiff.TrainPlan does).  With draw = 1, alpha_bar must hold at
 * least T entries (t is drawn in [0, T) and alpha_bar[t] read on the device).
 * draw = 0: t (B) / noise (B,P) are inputs.  draw = 1: the step draws them
 * itself into the same buffers (t ~ U{0..T-1}, noise ~ N(0,1), Philox4x32-10
 * keyed by (seed, member, step s): reproducible, independent of the grid).  */
int ertd_train_step_dev(const ertd_weights* w, const float* x0, int64_t* t, float* noise,
                        const float* cond, const float* alpha_bar, int B, int L, const float* freq,
                        float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                        int* step_dev, const float* adam_table, int table_first, int table_len,
                        int draw, int T, uint64_t seed, float* loss_out, void* ws, size_t ws_bytes,
                        void* stream);

/* nsteps consecutive ertd_train_step_dev steps (draw = 1 only: each step draws
 * its own t / noise from the device step count) in one call.  For graph
 * capture: a graph holding n steps of ONE call replays them back to back,
 * where n single-step calls captured one after another leave an ~8 us gap at
 * every call boundary of the graph (rocprofv3 trace, B = 32 -- measured, cause
 * in the runtime's graph, not in the kernels).  ertdiff.TrainPlan.run.  */
int ertd_train_steps_dev(const ertd_weights* w, const float* x0, int64_t* t, float* noise,
                         const float* cond, const float* alpha_bar, int B, int L, const float* freq,
                         float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                         int* step_dev, const float* adam_table, int table_first, int table_len,
                         int draw, int T, uint64_t seed, int nsteps, float* loss_out, void* ws,
                         size_t ws_bytes, void* stream);

/* One training epoch (:309-320 for every batch of the loader) from a dataset
 * resident on the device: x0_all (n_data,P), cond_all (n_data,14,L), and
 * rows (n_rows) int32 row indices into them -- the epoch's order; any indices
 * in [0, n_data), not necessarily a permutation.  The device cannot report a
 * bad index: THE CALLER CHECKS 0 <= rows[i] < n_data (ertdiff.TrainPlan.run_epoch
 * does).  Batch i takes rows[i*B .. min((i+1)*B, n_rows)); the last batch may
 * be partial and runs as a step of its own, smaller B (mean over B_last * P).
 * Each batch is one ertd_train_step_dev step -- the same four launches, the
 * kernels reading member b's x0 / cond through rows[i*B + b] -- with batch i's
 * t, noise and loss at t_all + i*B, noise_all + i*B*P and losses + i, so an
 * epoch step is bit for bit the step on the gathered batch, and a replay of a
 * captured graph of this call reads whatever order then sits in rows.
 * draw = 1: every step draws its t / noise (Philox keyed (seed, batch
 * position b, Adam step)) into its slice, so the epoch's draws are kept;
 * draw = 0: the slices are inputs.  losses: (ceil(n_rows / B)).  ws: the
 * ertd_workspace_bytes(B, L, P, 0, ERTD_OP_TRAIN) workspace.  Never allocates
 * or syncs.  step_dev / adam_table as for ertd_train_step_dev, including the
 * caveat: a step outside [table_first, table_first + table_len) is CLAMPED to
 * the nearest entry, so the table must cover all ceil(n_rows / B) steps.
 * ERTD_EINVAL for n_rows < 1, B < 1 or n_data < 1.                          */
int ertd_train_epoch_dev(const ertd_weights* w, const float* x0_all, const float* cond_all,
                         long long n_data, const int32_t* rows, int n_rows, int64_t* t_all,
                         float* noise_all, const float* alpha_bar, int B, int L, const float* freq,
                         float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                         int* step_dev, const float* adam_table, int table_first, int table_len,
                         int draw, int T, uint64_t seed, float* losses, void* ws, size_t ws_bytes,
                         void* stream);

/* One validation epoch (:327-338) over rows of the same resident dataset:
 * forward only -- no parameter, gradient or Adam state is written.  Per batch
 * i: eps = model(q_sample(x0, t, noise), t, cond) into eps_all + i*B*P and
 * losses[i] = MSELoss(mean)(eps, noise), summed in the train step's order.
 * draw = 1: the batch draws t / noise keyed (seed, batch position b, ctr[i]);
 * ctr (ceil(n_rows / B)) int32 on the device, filled by the caller with
 * values that differ for every batch and every call.  draw = 0: t_all /
 * noise_all are inputs (ctr may be NULL).  Same rows contract, workspace and
 * capture rules as ertd_train_epoch_dev.                                     */
int ertd_validation_epoch_dev(const ertd_weights* w, const float* x0_all, const float* cond_all,
                              long long n_data, const int32_t* rows, int n_rows, int64_t* t_all,
                              float* noise_all, const float* alpha_bar, int B, int L,
                              const float* freq, const int* ctr, int draw, int T, uint64_t seed,
                              float* eps_all, float* losses, void* ws, size_t ws_bytes,
                              void* stream);

/* The condition encoder's conv backward alone (the Conv1d part of
 * loss.backward(), :317), re-run on the state the last ertd_train_step /
 * ertd_train_step_dev / ertd_train_backward left in ws (same B, L, cond): it
 * rewrites the per-strip gradient rows in ws and nothing else.  For timing the
 * step's dominant kernel on its own (bench.py train_roofline).               */
int ertd_train_conv_backward(const float* cond, int B, int L, void* ws, size_t ws_bytes,
                             void* stream);

/* host: the Adam scalars of steps step_first ... step_first + n - 1 (6 floats
 * each), formed as torch.optim.Adam forms them (Python-float bias corrections). */
int ertd_adam_table(int step_first, int n, float lr, float beta1, float beta2, float eps,
                    float* out);

/* ---- build-defined conditional U-Net (SURVEY.md 8a'; north_star) -----------------
 * PARITY UNPINNED vs the reference: ERT_Conditional_Diffusion.py has no U-Net
 * (SURVEY.md 0.3).  The specification is oracle/unet_torch.py: x (B, image^2)
 * viewed as (B,1,image,image); emb = time MLP(sinusoid(t, ch)) + Linear(128->4ch)
 * of the reference's condition encoder (:133-142); ResBlocks of GroupNorm ->
 * SiLU -> 3x3 conv (+emb) -> GroupNorm -> SiLU -> 3x3 conv (+1x1 skip);
 * stride-2 Downsample, nearest-x2 Upsample + 3x3 conv, optional single-head
 * mid-block attention; GroupNorm -> SiLU -> 3x3 conv out.  fp32 throughout
 * (convs on fp32 MFMA).  Activations NCHW in the caller's workspace.         */
typedef struct ertd_unet_config {
  int image;       /* H = W: 16..128, power of two                          */
  int ch;          /* base channels                                         */
  int n_levels;    /* 1..4; every level >= 16x16                           */
  int ch_mult[4];  /* channel multiplier per level                          */
  int num_res;     /* ResBlocks per level on the way down (num_res+1 up)    */
  int attn;        /* 1: mid-block attention (needs 16x16 and C % 256 == 0) */
  int groups;      /* GroupNorm groups (32)                                 */
  int precision;   /* ERTD_PREC_FP32 (fp32 MFMA convs), ERTD_PREC_BF16
                      (bf16 conv operands, fp32 accumulate/activations) or
                      ERTD_PREC_BF16X3 (split-bf16 conv operands)          */
} ertd_unet_config;

/* Single U-Net operators (the SURVEY 8a' operator rows; used by per-operator
 * parity tests and microbenchmarks).
 * ertd_conv2d: out (B,Cout,Ho,Ho) = conv(act(cat(x (B,Ca,H,H), x2 (B,Cb,H,H))))
 *   + bias (+ ebias[b][co], row stride eb_stride) (+ res), ks 1|3, mode
 *   0 stride 1 / 1 stride 2 (Downsample) / 2 nearest-x2 upsample then conv;
 *   act 0 none / 1 GroupNorm+SiLU / 2 GroupNorm, gn = (B, Cin) float2
 *   {scale, shift} from ertd_group_norm_stats; precision FP32 | BF16 | BF16X3;
 *   H in {16,32,64,128} (Ho likewise); ws >= ertd_conv2d_workspace_bytes(Cin,
 *   Cout, ks, precision, B, H, mode): the packed weights plus the launch's
 *   scratch (a Winograd K split's partial sums, the bf16 pre-transformed
 *   input image), all caller-owned -- the call allocates nothing.  fp32 3x3 stride-1 convs with Cout % 64 == 0 run as
 *   Winograd F(4x4,3x3) (Cin, Ca % 4 == 0; H >= 32, or 16 when the tile items
 *   fill the device) or F(2x2,3x3) (Cin, Ca % 8 == 0), the rest as direct
 *   implicit GEMMs; ERTD_UNET_WINO=2 keeps F(2x2), 0 disables Winograd.
 * ertd_group_norm_stats: per (sample, channel) {gamma*rstd, beta-mean*gamma*rstd}
 *   of cat(x, x2) over `groups` groups (eps 1e-5), out (B, Ca+Cb) float2.
 * ertd_attention: qkv (B, 3C, N) -> out (B, C, N) = v softmax(q^T k / sqrt C)^T, N = 256.
 * ertd_group_norm_partials: parts (B, C, np, 2) = per (sample, channel, part of n = 256
 *   pixels) {sum, sum (x - sum/n)^2} of x (B, C, HW); HW = 256 np.  The fp32
 *   Winograd convs of the U-Net walk emit the same partials of their output from the
 *   epilogue, so a GroupNorm does not re-read its input.
 * ertd_group_norm_finalize: out (B, Ca+Cb) {scale, shift} exactly as ertd_group_norm_stats
 *   (and mr (B, groups) {mean, rstd}, optional) from the partials of the two concatenated
 *   inputs (pb = null when Cb = 0), combined per group in a fixed order in float64.  */
size_t ertd_conv2d_workspace_bytes(int cin, int cout, int ks, int precision, int B, int H,
                                   int mode);
int ertd_conv2d(const float* x, int Ca, const float* x2, int Cb, int B, int H, const float* w,
                const float* bias, int Cout, int ks, int mode, const float* gn, int act,
                const float* ebias, int eb_stride, const float* res, float* out, int precision,
                void* ws, size_t ws_bytes, void* stream);
/* ertd_conv2d_run: the same conv reusing the packing a previous ertd_conv2d call with the
 * same (Ca, Cb, B, H, Cout, ks, mode, act, precision) and weights left at the head of ws
 * (no weight read, no pack kernel: the conv kernel alone, e.g. for per-kernel timing). */
int ertd_conv2d_run(const float* x, int Ca, const float* x2, int Cb, int B, int H, const float* bias,
                    int Cout, int ks, int mode, const float* gn, int act, const float* ebias,
                    int eb_stride, const float* res, float* out, int precision, void* ws,
                    size_t ws_bytes, void* stream);
/* ertd_conv2d_gn_parts: np > 0 when the fp32 conv ertd_conv2d dispatches for this geometry
 *   emits the GroupNorm partials of its output from the epilogue ((B, Cout, np) float2
 *   {sum, M2} over HW / np pixels each, the ertd_group_norm_partials format), else 0.
 * ertd_conv2d_gn / ertd_conv2d_run_gn: ertd_conv2d / ertd_conv2d_run that also write those
 *   partials (gn_np = that np), for ertd_group_norm_finalize without re-reading the output
 *   (the train walk).  */
int ertd_conv2d_gn_parts(int Ca, int Cb, int Cout, int ks, int mode, int act, int precision, int B, int H);
int ertd_conv2d_gn(const float* x, int Ca, const float* x2, int Cb, int B, int H, const float* w,
                   const float* bias, int Cout, int ks, int mode, const float* gn, int act,
                   const float* ebias, int eb_stride, const float* res, float* out, int precision,
                   void* ws, size_t ws_bytes, float* gn_parts, int gn_np, void* stream);
int ertd_conv2d_run_gn(const float* x, int Ca, const float* x2, int Cb, int B, int H, const float* bias,
                       int Cout, int ks, int mode, const float* gn, int act, const float* ebias,
                       int eb_stride, const float* res, float* out, int precision, void* ws,
                       size_t ws_bytes, float* gn_parts, int gn_np, void* stream);
/* ertd_conv2d_route_info: which kernel an ertd_conv2d call with this geometry
 *   dispatches and how it is laid over the device -- a read-only query that
 *   launches nothing, computed by the dispatch functions the launch itself
 *   runs (so it holds for the device's CU count and the library's defaults).
 *   has_ebias: bit 0 = the call has an ebias operand, bit 1 = a res operand
 *   (operands some kernels do not take).  Returns ERTD_OK, or ERTD_EINVAL for
 *   a geometry ertd_conv2d rejects.
 *   kernel   ERTD_ROUTE_*;
 *   ksplit   2: a Winograd layer's input channels run as two half-items, else 1;
 *   items, grid   persistent kernels (the Winograd convs, the skip GEMM): work
 *            items of the launch and its workgroups; workgroup g runs items g,
 *            g + grid, ... (in the F4S kernel's XCD-aware order where it takes
 *            it), so with items > grid and items % grid != 0 neighbouring
 *            workgroups run different numbers of items.  0, 0 otherwise;
 *   gn_parts what ertd_conv2d_gn_parts returns for the call.
 * Placement invariance (the persistent kernels' contract): a sample's output
 *   bits depend on that sample's operands and on the route -- (kernel, ksplit,
 *   tile), a function of the geometry and B -- and on nothing else: not on the
 *   sample's position in the batch, hence not on the item, the round or the
 *   workgroup that computes it, nor on how many items that workgroup runs.
 *   Permuting the samples of a batch permutes the output bit for bit.  (The
 *   skip GEMM's tile does not depend on B either: there a sample's bits do not
 *   depend on the batch at all.)  */
#define ERTD_ROUTE_DIRECT 0           /* implicit GEMM (1x1 / 3x3, any stride)      */
#define ERTD_ROUTE_CONV_IN 1          /* Cin = 1 3x3                                */
#define ERTD_ROUTE_CONV_OUT 2         /* Cout = 1 3x3                               */
#define ERTD_ROUTE_UP 3               /* sub-pixel Upsample conv                    */
#define ERTD_ROUTE_CONV1X1 4          /* 1x1, LDS-DMA                               */
#define ERTD_ROUTE_SKIP_GEMM 5        /* reserved (the fp32 MFMA GEMM): not reported */
#define ERTD_ROUTE_SKIP_GEMM_SPLIT 6  /* 1x1 batched GEMM, split-bf16 MFMA          */
#define ERTD_ROUTE_F2 7               /* Winograd F(2x2,3x3)                        */
#define ERTD_ROUTE_F4 8               /* Winograd F(4x4,3x3), weights in LDS        */
#define ERTD_ROUTE_F4S 9              /* Winograd F(4x4,3x3), weights in registers  */
#define ERTD_ROUTE_F4S_UP 10          /* ... on the nearest-x2 source (Upsample)    */
#define ERTD_ROUTE_BF16 11            /* the bf16 / split-bf16 operand convs        */
typedef struct ertd_route_info {
  int kernel;
  int ksplit;
  int items, grid;
  int gn_parts;
} ertd_route_info;
int ertd_conv2d_route_info(int Ca, int Cb, int Cout, int ks, int mode, int act, int precision,
                           int has_ebias, int B, int H, ertd_route_info* out);
int ertd_group_norm_stats(const float* x, int Ca, const float* x2, int Cb, int B, int HW,
                          int groups, const float* gamma, const float* beta, float* out,
                          void* stream);
int ertd_attention(const float* qkv, int B, int C, int N, float* out, void* stream);
int ertd_group_norm_partials(const float* x, int C, int B, int HW, int np, float* parts, void* stream);
int ertd_group_norm_finalize(const float* pa, int npa, int Ca, const float* pb, int npb, int Cb, int B,
                             int HW, int groups, const float* gamma, const float* beta, float* out,
                             float* mr, void* stream);
/* ertd_act_bf16: img [B][ceil(C/16)][Ho][Ho][16] bf16 (RNE) of act(cat(x, x2)*ss.x + ss.y)
 *   (act 0 none / 1 GN+SiLU / 2 GN; ss (B, C, 2) as ertd_group_norm_stats) or, with up = 1
 *   (act 0), of the nearest-x2 upsample of cat(x, x2) (Ho = 2H): the bf16 path's standalone
 *   image transform (act_bf16_kernel).
 * ertd_unet_update: the U-Net sampler's DDPM update (sample_model :111-118) of x (B, P) given
 *   eps, per-step tables c1/c2/sigma (index t = *t_dev) and injected noise
 *   (num_steps, B, P) or Philox (noise = null; seed, member ids from member_offset). */
int ertd_act_bf16(const float* x, int Ca, const float* x2, int Cb, int B, int H, const float* ss,
                  int act, int up, void* img, void* stream);
int ertd_unet_update(float* x, const float* eps, const float* c1, const float* c2,
                     const float* sigma, const float* noise, int num_steps, const int* t_dev,
                     uint64_t seed, uint32_t member_offset, int B, int P, void* stream);
/* ertd_group_norm_act_bf16: the bf16 path's fused prologue of a 3x3 GN conv
 *   in one pass -- out as ertd_group_norm_stats, and img = bf16 RNE of
 *   act(GroupNorm(cat(x, x2))) (act: silu=1 SiLU, 0 none) in the conv's
 *   [B][C/16][H][H][16] layout (C*H*H*2 bytes per sample).  ERTD_EINVAL
 *   unless C % 16 == 0, lcm(C/groups, 16) * H*H <= 65536 (and a multiple of
 *   1024), H*H % 64 == 0.                                                    */
int ertd_group_norm_act_bf16(const float* x, int Ca, const float* x2, int Cb, int B, int H,
                             int groups, const float* gamma, const float* beta, float* out,
                             void* img, int silu, void* stream);

/* Parameter tensors in state_dict order: count, and (name, shape) of one.  */
int ertd_unet_n_params(const ertd_unet_config* cfg);
int ertd_unet_param_info(const ertd_unet_config* cfg, int idx, char* name, int name_len,
                         int64_t* shape, int* ndim);
/* Packed device weights (floats) and their packing from the params array
 * (ertd_unet_n_params device pointers, state_dict order).  freq: (ch/2)
 * float32 sinusoid frequencies computed on the host with the reference's
 * get_timestep_embedding expression (:80-88) at dim = ch.                 */
size_t ertd_unet_packed_floats(const ertd_unet_config* cfg);
int ertd_unet_pack(const ertd_unet_config* cfg, const float* const* params, const float* freq,
                   float* packed, void* stream);
/* Workspace bytes for batch B and condition length L (forward and sampler). */
size_t ertd_unet_workspace_bytes(const ertd_unet_config* cfg, int B, int L);
/* eps = unet(x (B, image^2), t (B,) int64, cond (B,14,L) with member stride
 * cond_stride floats (0: one shared condition)); cond_emb_out (B,128) optional. */
int ertd_unet_forward(const ertd_unet_config* cfg, const float* packed, const float* x,
                      const int64_t* t, const float* cond, long long cond_stride, int L, int B,
                      float* out, float* cond_emb_out, void* ws, size_t ws_bytes, void* stream);
/* sample_model (:102-119) around the U-Net: steps t = t_first .. t_first-n_run+1 on
 * x_inout (B, image^2); c1/c2/sigma/noise/seed/member_offset as in ertd_sample.
 * The condition embedding is computed once per call (it does not depend on x
 * or t; recomputing it per step would give identical bits).               */
int ertd_unet_sample(const ertd_unet_config* cfg, const float* packed, const float* cond,
                     long long cond_stride, int L, int B, int num_steps, int t_first, int n_run,
                     const float* c1, const float* c2, const float* sigma, const float* noise,
                     uint64_t seed, uint32_t member_offset, float* x_inout, void* ws,
                     size_t ws_bytes, void* stream);
/* The same call as a plan: the head and one step are captured as hipGraphs
 * once; a launch replays head + n_run x step on `stream`.  For bf16
 * precision the step graph is not a single chain: the embedding dense layers
 * and each ResBlock's 1x1 skip conv are captured on a plan-owned side stream
 * (event fork/join), so they run beside conv_in / conv1 (fp32 captures one
 * chain: its persistent Winograd convs occupy every CU); results equal the
 * eager call bit for bit either way.  The plan owns its capture streams and
 * events (ertd_unet_plan_destroy frees them); ERTD_UNET_SIDE=0/1 in the
 * environment forces one chain / the forked graph.                          */
typedef struct ertd_unet_plan ertd_unet_plan;
int ertd_unet_sample_plan_create(const ertd_unet_config* cfg, const float* packed, const float* cond,
                                 long long cond_stride, int L, int B, int num_steps, int t_first,
                                 int n_run, const float* c1, const float* c2, const float* sigma,
                                 const float* noise, uint64_t seed, uint32_t member_offset,
                                 float* x_inout, void* ws, size_t ws_bytes, ertd_unet_plan** plan);
/* ertd_sample_solver around the U-Net: steps k = k_first .. k_first+n_run-1 of
 * the K-step table on x_inout (B, image^2); timesteps / coef / clip / noise /
 * seed / member_offset as there.  d_prev_inout (B, image^2) is required: the
 * update kernel stores D every step (and reads it only when c_k != 0).  The
 * workspace is ertd_unet_workspace_bytes, unchanged: the step counter slot
 * holds two words, {tau_k, k}.                                             */
int ertd_unet_sample_solver(const ertd_unet_config* cfg, const float* packed, const float* cond,
                            long long cond_stride, int L, int B, int K, int k_first, int n_run,
                            const int32_t* timesteps, const float* coef, float clip,
                            const float* noise, uint64_t seed, uint32_t member_offset,
                            float* x_inout, float* d_prev_inout, void* ws, size_t ws_bytes,
                            void* stream);
/* The same call as a plan (ertd_unet_plan_launch / _launch_steps / _destroy):
 * the tables are checked once here, on `stream`; the step graph is captured
 * once and replayed n_run times, reading {tau_k, k} from the two device
 * words, which a word kernel at the end of the step advances from the device
 * timesteps table.  Equal to the eager call bit for bit.                   */
int ertd_unet_sample_solver_plan_create(const ertd_unet_config* cfg, const float* packed,
                                        const float* cond, long long cond_stride, int L, int B,
                                        int K, int k_first, int n_run, const int32_t* timesteps,
                                        const float* coef, float clip, const float* noise,
                                        uint64_t seed, uint32_t member_offset, float* x_inout,
                                        float* d_prev_inout, void* ws, size_t ws_bytes,
                                        void* stream, ertd_unet_plan** plan);
int ertd_unet_plan_launch(ertd_unet_plan* plan, void* stream);
/* head + the first n_steps (0 <= n_steps <= n_run) steps only: warms both
 * graphs (first-launch upload) without running the whole plan.            */
int ertd_unet_plan_launch_steps(ertd_unet_plan* plan, int n_steps, void* stream);
int ertd_unet_plan_destroy(ertd_unet_plan* plan);

/* ---- U-Net training operators (csrc/unet_train.hip; the reference train step
 * ERT_Conditional_Diffusion.py:305-320 around the build-defined U-Net, walked
 * by ertdiff/unet_train.py).  PARITY UNPINNED vs the reference (no U-Net
 * there): checked against torch autograd on oracle/unet_torch.py.  All device
 * pointers, enqueued on `stream`; `accumulate` = add into the output.
 * ertd_gn_stats_mr: ertd_group_norm_stats + mr_out (B, groups) {mean, rstd}.
 * ertd_gn_act_apply: out (B, Ca+Cb, HW) = act(cat(x, x2) * ss.x + ss.y), act 1 GN+SiLU / 2 GN.
 * ertd_gn_act_backward: dx / dx2 of act(GroupNorm(cat(x, x2))) given dy (B, C, HW);
 *   dgb_part (B, 2, C): per-sample sum dxn*xhat ([b][0]) and sum dxn ([b][1]) ->
 *   (dgamma | dbeta) by one ertd_reduce_rows (rows B, cols 2C).
 * ertd_gn_act_backward_csum: the same, plus csum[b * ldc + c] = sum over the HW pixels
 *   of the gradient this call adds to channel c of sample b (a ResBlock's emb-projection
 *   gradient when dx is the conv1 output's gradient; channels per group <= 64).
 * ertd_gn_act_backward_add: the same with an addend: dx / dx2 (+)= addc + the GroupNorm
 *   gradient, addc (B, C, HW) in the concatenated channel order (a ResBlock's skip / identity
 *   gradient of the same input), added first (as a separate add before the call would); csum
 *   optional (null: none), and when given it sums the GroupNorm term only.
 * ertd_im2col: out (B, C*ks*ks, Ho*Ho) patches of x (B, C, H, H), mode 0 s1 / 1 s2 (even H,
 *   Ho = H / 2) / 2 upsample.
 * ertd_wgrad_gemm: dW (M, N) = sum_b dY_b (M, P) . X_b (N, P)^T (batch strides bsA, bsB),
 *   fp32 MFMA, split per sample + fixed-order reduction; ws >= ertd_wgrad_ws_bytes.
 * ertd_conv_weight_flip: out (Cin, Cout, ks, ks) = w (Cout, Cin, ks, ks) spatially flipped.
 * ertd_zero_insert: out (B, C, 2Ho, 2Ho) with x at even positions; ertd_sum_pool2: 2x2 sums.
 * ertd_channel_sums: out_bc (B, C; row stride ldo, 0 = C) sums over HW; out_c (C) = sum over b
 *   (optional, ldo = C).
 * ertd_concat: dst = cat(srcs[0..n)) of contiguous fp32 tensors (sizes in elements).
 * ertd_encoder_train_pack: copies condition_encoder.0 / .2 weights into an
 *   ertd_packed_floats() buffer (the layout ertd_encoder_train_fwd / _bwd read).
 * ertd_gemm_small: C[b][i][j] = alpha sum_k A[b][i][k] B[b][k][j] (+ bias[j]) with element
 *   strides (a_i, a_k, a_b, b_k, b_j, b_b, c_i, c_j, c_b).
 * ertd_softmax_rows: P = softmax(scale S) per row; ertd_softmax_backward: dS = scale P (dP - <dP, P>).
 * ertd_eltwise: op 0 silu(x), 1 y silu'(x), 2 relu(x), 3 y [x > 0], 4 x + y, 5 alpha x.
 * ertd_channel_slice: dst (B, Cdst, HW) channels [d0, d0+Cd) (+)= src (B, Cs, HW) channels
 *   [c0, c0+Cd).
 * ertd_mse_loss: loss (1) = mean (eps - noise)^2, dout = 2 (eps - noise) / n (optional);
 *   ws >= ertd_mse_loss_ws_bytes() (float64 partial sums, caller-owned).
 * ertd_encoder_train_fwd / _bwd: the reference condition encoder (:133-142) with saved
 *   activations in ws (pool mean m (B, 64) out) / conv-parameter grads from g = dL/dm / L.
 * ertd_adam_multi: torch.optim.Adam step (no weight decay) over ntensors tensors; lr, betas
 *   and eps as doubles (the optimizer's Python floats: 1 - beta2 is formed in double).  */
int ertd_gn_stats_mr(const float* x, int Ca, const float* x2, int Cb, int B, int HW, int groups,
                     const float* gamma, const float* beta, float* ss_out, float* mr_out,
                     void* stream);
int ertd_gn_act_apply(const float* x, int Ca, const float* x2, int Cb, int B, int HW,
                      const float* ss, int act, float* out, void* stream);
int ertd_gn_act_backward(const float* x, int Ca, const float* x2, int Cb, int B, int HW, int groups,
                         const float* gamma, const float* beta, const float* mr, int act,
                         const float* dy, float* dx, float* dx2, int accumulate, float* dgb_part,
                         void* stream);
int ertd_gn_act_backward_csum(const float* x, int Ca, const float* x2, int Cb, int B, int HW, int groups,
                              const float* gamma, const float* beta, const float* mr, int act,
                              const float* dy, float* dx, float* dx2, int accumulate, float* dgb_part,
                              float* csum, long long ldc, void* stream);
int ertd_gn_act_backward_add(const float* x, int Ca, const float* x2, int Cb, int B, int HW, int groups,
                             const float* gamma, const float* beta, const float* mr, int act,
                             const float* dy, const float* addc, float* dx, float* dx2, int accumulate,
                             float* dgb_part, float* csum, long long ldc, void* stream);
int ertd_im2col(const float* x, int C, int B, int H, int ks, int mode, float* out, void* stream);
size_t ertd_wgrad_ws_bytes(int M, int N, int P, int B);
int ertd_wgrad_gemm(const float* dY, const float* X, int M, int N, int P, int B, long long bsA,
                    long long bsB, float* dW, int accumulate, void* ws, size_t ws_bytes,
                    void* stream);
int ertd_reduce_rows(const float* part, int rows, long long cols, float* out, int accumulate,
                     void* stream);
/* ertd_reduce_rows_multi: n independent ertd_reduce_rows problems (host arrays of
 * their arguments) in ceil(n / 48) launches; every output bitwise equal to the
 * single call's.  The U-Net train walk defers its per-layer dgamma/dbeta and
 * linear-bias reductions (no other kernel reads them before the optimizer) to one
 * such call at the end of the backward.                                         */
int ertd_reduce_rows_multi(const float* const* parts, const int* rows, const long long* cols,
                           float* const* outs, const int* accumulate, int n, void* stream);
int ertd_conv_weight_flip(const float* w, int Cout, int Cin, int ks, float* out, void* stream);
int ertd_zero_insert(const float* x, int B, int C, int Ho, float* out, void* stream);
int ertd_sum_pool2(const float* x, int B, int C, int H, float* out, int accumulate, void* stream);
int ertd_channel_sums(const float* x, int B, int C, int HW, float* out_bc, int ldo, float* out_c,
                      int accumulate_c, void* stream);
int ertd_gemm_small(const float* A, long long a_i, long long a_k, long long a_b, const float* Bm,
                    long long b_k, long long b_j, long long b_b, float* C, long long c_i,
                    long long c_j, long long c_b, const float* bias, int I, int J, int K, int batch,
                    float alpha, int accumulate, void* stream);
int ertd_softmax_rows(const float* S, long long rows, int N, float scale, float* P, void* stream);
int ertd_softmax_backward(const float* P, const float* dP, long long rows, int N, float scale,
                          float* dS, void* stream);
int ertd_eltwise(int op, const float* x, const float* y, float* out, long long n, float alpha,
                 int accumulate, void* stream);
int ertd_channel_slice(const float* src, int B, int Cs, int c0, int Cd, int HW, float* dst,
                       int Cdst, int d0, int accumulate, void* stream);
size_t ertd_mse_loss_ws_bytes(void);
int ertd_mse_loss(const float* eps, const float* noise, long long n, float* loss, float* dout,
                  void* ws, size_t ws_bytes, void* stream);
/* ertd_conv_wgrad: dW (Cout, Ca+Cb, ks, ks) (+)= the weight gradient of
 *   y = conv(cat(x, x2)) (mode 0 stride 1 / 1 stride 2 / 2 nearest-x2 upsample,
 *   as ertd_conv2d) given dy (B, Cout, Ho, Ho): implicit GEMM on fp32 MFMA,
 *   fixed-order split reduction; ws >= ertd_conv_wgrad_ws_bytes (0 = unsupported
 *   geometry: output side not a power of two in [16, 128]).  csrc/unet_wgrad.hip. */
size_t ertd_conv_wgrad_ws_bytes(int Cin, int Cout, int B, int H, int ks, int mode);
/* ertd_conv_input_grad: dx (B, Cin, H, H) (+)= dL/dx of y = conv(x) (weight w (Cout, Cin, ks, ks),
 *   mode as ertd_conv2d) given dy (B, Cout, Ho, Ho): a stride-1 conv of dy (stride 2:
 *   zero-inserted; upsample: at 2H then 2x2 sum-pooled) with w transposed and flipped, packed
 *   straight from w (Winograd where eligible); ws >= ertd_conv_input_grad_ws_bytes.       */
size_t ertd_conv_input_grad_ws_bytes(int Cin, int Cout, int B, int H, int ks, int mode);
int ertd_conv_input_grad(const float* dy, int B, int H, const float* w, int Cout, int Cin, int ks,
                         int mode, float* dx, int accumulate, void* ws, size_t ws_bytes,
                         void* stream);
/* ertd_conv_input_grad_run: the same, reusing the flipped packing an earlier
 *   ertd_conv_input_grad (or ertd_conv_pack_batch with the descriptor of
 *   ertd_conv_input_grad_pack_desc) left at the head of ws.                    */
int ertd_conv_input_grad_run(const float* dy, int B, int H, int Cout, int Cin, int ks, int mode,
                             float* dx, int accumulate, void* ws, size_t ws_bytes, void* stream);
int ertd_conv_wgrad(const float* dy, const float* x, int Ca, const float* x2, int Cb, int B, int H,
                    int Cout, int ks, int mode, const float* gn, int act, float* dw, int accumulate,
                    void* ws, size_t ws_bytes, void* stream);
/* ertd_conv_wgrad_bias: ertd_conv_wgrad plus the conv's bias gradient db (Cout) = sum of dy
 *   over samples and pixels (written, not accumulated; also into db2 when non-null, e.g.
 *   a 1x1 skip conv fed the same dy), fused into the Winograd path's dy transform.  Only
 *   where ertd_conv_wgrad_bias_ok (3x3 stride 1 / upsample on the Winograd path, B * tiles
 *   a multiple of 256); ws as ertd_conv_wgrad_ws_bytes.                                  */
int ertd_conv_wgrad_bias_ok(int Cin, int Cout, int B, int H, int ks, int mode);
int ertd_conv_wgrad_bias(const float* dy, const float* x, int Ca, const float* x2, int Cb, int B, int H,
                         int Cout, int ks, int mode, const float* gn, int act, float* dw, int accumulate,
                         float* db, float* db2, void* ws, size_t ws_bytes, void* stream);

/* Batched fp32 weight packing (the train step packs every conv once per
 * optimizer step, in one launch).  A descriptor names one packing: the source
 * weight, its destination, and the layout a later ertd_conv2d_run /
 * ertd_conv_input_grad_run on that workspace reads -- filled by the two
 * *_pack_desc queries from the same dispatch decisions as ertd_conv2d /
 * ertd_conv_input_grad, so the batch writes exactly their packings, bit for bit. */
#define ERTD_PACK_DIRECT 0 /* implicit-GEMM fragment order (1x1 / 3x3)   */
#define ERTD_PACK_UP 1     /* sub-pixel Upsample classes                 */
#define ERTD_PACK_WINO 2   /* Winograd F(2x2,3x3) U = G g G^T            */
#define ERTD_PACK_WINO4 3  /* Winograd F(4x4,3x3)                        */
typedef struct {
  const float* w;      /* source weight (Cout, Cin, ks, ks) of the FORWARD conv    */
  float* dst;          /* destination (inside the conv's workspace)               */
  long long total;     /* packed floats                                           */
  int cin, cout, ks;   /* of the packed conv (flip: the input-gradient conv's)    */
  int kind;            /* ERTD_PACK_*                                             */
  int flip;            /* 1: the input-gradient conv's transposed, flipped weight */
  int nchunk;          /* K chunks of the layout                                  */
  int block0;          /* first 256-thread block (ertd_conv_pack_batch_prepare)   */
  int reserved;        /* set by the *_pack_desc queries (ERTD_PACK_WINO4: 1 = the      */
                       /* Upsample conv's point set); pass it on unchanged              */
} ertd_pack_desc;
int ertd_conv2d_pack_desc(int Cin, int Ca, int Cout, int ks, int mode, int precision, int B, int H,
                          const float* w, void* ws, ertd_pack_desc* out);
int ertd_conv_input_grad_pack_desc(int Cin, int Cout, int B, int H, int ks, int mode, const float* w,
                                   void* ws, ertd_pack_desc* out);
/* host: fills block0 of descs[0..n) in order; returns the batch's block count (< 0: error) */
int ertd_conv_pack_batch_prepare(ertd_pack_desc* descs, int n);
/* one launch packing all n descriptors (descs: DEVICE copy of the prepared table) */
int ertd_conv_pack_batch(const ertd_pack_desc* descs, int n, int blocks, void* stream);
int ertd_concat(const float* const* srcs, const long long* sizes, int n, float* dst, void* stream);
/* ertd_split: dsts[k] = alpha * src[sum(sizes[<k]) ...] (the inverse of ertd_concat, scaled):
 *   the data-parallel train step's gradient bucket back into the per-tensor gradients. */
int ertd_split(const float* src, float* const* dsts, const long long* sizes, int n, float alpha,
               void* stream);
int ertd_encoder_train_pack(const float* w0, const float* w2, float* packed, void* stream);
size_t ertd_encoder_train_ws_bytes(int B, int L);
int ertd_encoder_train_fwd(const float* packed, const float* b1, const float* b2, const float* cond,
                           int B, int L, float* m_out, void* ws, size_t ws_bytes, void* stream);
int ertd_encoder_train_bwd(const float* packed, const float* cond, const float* g, int B, int L,
                           float* dw1, float* db1, float* dw2, float* db2, void* ws,
                           size_t ws_bytes, void* stream);
int ertd_adam_multi(float* const* params, const float* const* grads, float* const* exp_avg,
                    float* const* exp_avg_sq, const long long* sizes, int ntensors, int step,
                    double lr, double beta1, double beta2, double eps, void* stream);

/* ---- Ensemble KDE mode (csrc/kde.hip) -------------
 * Replaces the reference's per-cell loop ERT_Conditional_Diffusion.py:747-762
 * (scipy.stats.gaussian_kde per cell of sim_data, evaluated on
 * np.linspace(lo, hi, grid), mode = grid point of the first maximum) and
 * mode_kde_calculation :166-181 (one array, its own range, 1000 points).
 * x: (n, ld) float64 row-major on the device, cell c = column c < cells.
 * range_mode 0: grid over [lo, hi]; 1: each cell's own [min, max];
 * 2: [lo, hi] read from range_dev (2 doubles, e.g. ertd_minmax_f64's output).
 * mode (cells) receives the mode; index (cells, optional) the grid index, -1
 * where the cell's variance is 0 (gaussian_kde raises there); density
 * (cells, optional) the KDE value at the mode.  Requires 2 <= n <= 20480.   */
int ertd_kde_mode(const double* x, int n, long long cells, long long ld, int grid, int range_mode,
                  double lo, double hi, const double* range_dev, double* mode, int* index,
                  double* density, void* stream);

/* min and max of count float64 values: out2 = {min, max} (device);
 * work: 2 * ERTD_MINMAX_BLOCKS doubles of device scratch.                  */
#define ERTD_MINMAX_BLOCKS 1024
int ertd_minmax_f64(const double* x, long long count, double* work, double* out2, void* stream);

/* ---- Ensemble order statistics, coverage, moments, WSSE (csrc/ensstats.hip) ----
 * Replaces the host numpy the reference runs on the sampler's and the
 * simulator's ensembles: ERT_Conditional_Diffusion.py:867-876 (per-cell mean,
 * std, variance, P25/P50/P75), :1121-1132 and :1191-1205 (60 np.percentile
 * calls, the coverage indicator and its mean per level) and :767-787 (WSSE).
 * Every entry point takes float32 or float64 input (dtype) and computes in
 * float64.  x: (n, ld) row-major on the device, cell c = column c < cells
 * (the layout of the KDE entry point above).
 * valid_rows (optional): uint8 (n, cells / rows_per_valid), the mask that
 * postprocessing writes -- one entry covers the rows_per_valid adjacent
 * columns of a test sample; cells must be a multiple of rows_per_valid.  A
 * column's used samples are the m rows whose entry is set (m = n without a
 * mask).                                                                    */
#define ERTD_F32 0
#define ERTD_F64 1
/* Percentiles of every column, bit for bit np.percentile(x, 100 q, axis=0)
 * (method "linear"): with s the sorted used samples, vi = (m-1) q[k],
 * lo = floor(vi), hi = min(lo+1, m-1), t = vi - lo, d = s[hi] - s[lo] formed
 * in the input's dtype, out[k, c] = t < 0.5 ? s[lo] + d t : s[hi] - d (1-t)
 * in float64.  q: nq float64 fractions in [0, 1] on the device; out: (nq,
 * cells) float64; n_eff (cells, optional) receives m.  A column with m = 0,
 * or with a NaN among its used samples, yields NaN.  Requires
 * 1 <= n <= 16384 (one workgroup sorts a whole column in LDS).              */
int ertd_ens_percentile(const void* x, int dtype, int n, long long cells, long long ld,
                        const unsigned char* valid_rows, int rows_per_valid, const double* q,
                        int nq, double* out, int* n_eff, void* stream);
/* Mean and population variance (ddof = 0) of every column, two passes:
 * mean[c] = sum(x) / m, var[c] = sum((x - mean)^2) / m, each (cells) float64.
 * m = 0 yields NaN.  n >= 1.                                                */
int ertd_ens_moments(const void* x, int dtype, int n, long long cells, long long ld,
                     const unsigned char* valid_rows, int rows_per_valid, double* mean,
                     double* var, void* stream);
/* The calibration loop in one launch.  ens: (S, N, P); truth: (N, P), same
 * dtype; q_low, q_upp: K float64 fractions (device), the bounds of K central
 * intervals.  Per column (i, p) the two bounds are the percentiles above and
 * counts[k, p] += (low < truth) & (truth <= upp), compared in float64;
 * cols[p] += 1 for every column with m >= 1 (columns with m = 0 enter
 * neither).  counts (K, P) and cols (P) are int32 and are zeroed by the call;
 * integer accumulation, so the result is deterministic and the counts of
 * disjoint slices of N add up.  valid_rows (optional): (S, N).
 * Requires 1 <= S <= 16384 and (K + 1) P <= 4096.                           */
int ertd_coverage(const void* ens, const void* truth, int dtype, int S, long long N, int P,
                  const unsigned char* valid_rows, const double* q_low, const double* q_upp, int K,
                  int* counts, int* cols, void* stream);
/* WSSE per realisation and survey: pred (n, M, E), obs (M, E), same dtype;
 * out[s, e] = mean over m of (pred - obs)^2 / (A |obs| + B)^2, (n, E) float64. */
int ertd_wsse(const void* pred, const void* obs, int dtype, int n, long long M, int E, double A,
              double B, double* out, void* stream);

/* ---- Row sort and Wasserstein-1 distance (csrc/rowsort.hip) -------------------
 * Replaces the host scipy.stats.wasserstein_distance the reference calls on
 * a flattened simulated ERT image and the flattened conditional observation:
 * ERT_Conditional_Diffusion.py:860 (each of the best simulations) and
 * :898-899 (the ensemble mean and mode), 65,702 values per side.  Rows are
 * contiguous, row s at x + s * ld (ld >= M), float32 or float64 (dtype); a
 * row is sorted by many workgroups: LDS tile sorts, then merge passes in
 * global memory between `out` and the caller's workspace.  Deterministic; no
 * allocation, no host synchronisation.  Both calls require n >= 1,
 * 1 <= M <= 2^24 and n * ceil(M / 1024) <= 2^22, and return ERTD_EINVAL
 * otherwise, ERTD_ENOSPC for a workspace shorter than the _ws_bytes call
 * reports (0 for arguments the call would reject).                          */
/* keys per LDS tile for this dtype (tests build their edge shapes from it);
 * 0 for an unknown dtype                                                    */
int ertd_rows_sort_tile(int dtype);
size_t ertd_rows_sort_ws_bytes(int dtype, int n, long long M);
/* out (n, M) contiguous, input dtype: every row ascending, NaNs last (the
 * order of np.sort).  x and out may not overlap.  ws may be null where
 * ertd_rows_sort_ws_bytes is 0 (rows of one tile).                          */
int ertd_rows_sort(const void* x, int dtype, int n, long long M, long long ld, void* out,
                   void* ws, size_t ws_bytes, void* stream);
size_t ertd_wasserstein_ws_bytes(int dtype, int n, long long Mu, long long Mv);
/* out (n) float64: W1(row s of u, v); u (n, Mu) pitch ld, v (Mv), same dtype.
 * scipy's _cdf_distance(p = 1) without weights, term for term: both sides
 * sorted in their dtype, promoted to float64, and with z the merged sorted
 * sequence, i_k / j_k the keys of u / v among z[0..k],
 *   out[s] = sum over k < Mu + Mv - 1 of |i_k / Mu - j_k / Mv| (z[k+1] - z[k])
 * with two real divisions per term, so each term carries scipy's bits; the
 * terms are added in a fixed order (chains of at most 64, a term passes
 * through at most 88 additions).  A NaN in row s makes out[s] NaN, a NaN in
 * v every out[s].                                                            */
int ertd_wasserstein(const void* u, int dtype, int n, long long Mu, long long ld,
                     const void* v, long long Mv, double* out,
                     void* ws, size_t ws_bytes, void* stream);

/* ---- MinMax scaling and the training set on the device (csrc/dataprep.hip) ----
 * Replaces the host sklearn / numpy of the reference's scaling cell
 * ERT_Conditional_Diffusion.py:230-269 (MinMaxScaler.fit_transform of the
 * (5076, 65702) float64 ERT array and of the (5076, 29) parameters, then
 * DiffusionDataset's transpose :72 and .float()) and of :417-419
 * (ert_scaler.inverse_transform of float32 conditions after a swapaxes).
 * Every float64 operation is one separately rounded IEEE operation in
 * sklearn 1.7's order, so the results equal sklearn's bit for bit.  All
 * arrays are on the device; X is row-major with a row pitch of ldx values.
 * No allocation, no host synchronisation.                                   */
/* Workspace of ertd_minmax_partial_fit: the per-slab column minima and maxima
 * (0 for arguments the call would reject).                                  */
size_t ertd_minmax_ws_bytes(long long n, long long F);
/* data_min[f] = np.nanmin(X[:, f]), data_max[f] = np.nanmax(X[:, f]) over the
 * n rows: a NaN is skipped, an all-NaN column yields NaN.  accumulate != 0:
 * the result is then combined with the values already in data_min /
 * data_max by np.minimum / np.maximum (which propagate a NaN) -- one
 * MinMaxScaler.partial_fit call after the first.  16-byte loads when F and
 * ldx are even and X is 16-byte aligned, 8-byte loads otherwise.            */
int ertd_minmax_partial_fit(const double* X, long long n, long long F, long long ldx,
                            double* data_min, double* data_max, int accumulate, void* ws,
                            size_t ws_bytes, void* stream);
/* The fitted vectors for feature_range (fr0, fr1), each (F) float64:
 *   range  = data_max - data_min                      (data_range_; optional)
 *   scale  = (fr1 - fr0) / (range < 10 DBL_EPSILON ? 1 : range)   (scale_)
 *   min_   = fr0 - data_min * scale                   (min_)
 * A NaN range stays NaN (the comparison is false), as in sklearn.           */
int ertd_minmax_finalize(const double* data_min, const double* data_max, long long F, double fr0,
                         double fr1, double* scale, double* min_, double* range, void* stream);
/* MinMaxScaler.transform in float64: out[i, f] = X[i, f] * scale[f] + min_[f],
 * the product and the sum each rounded.  out (row pitch ldo) may be X.      */
int ertd_minmax_transform(const double* X, long long n, long long F, long long ldx,
                          const double* scale, const double* min_, double* out, long long ldo,
                          void* stream);
/* MinMaxScaler.inverse_transform in X's dtype (ERTD_F32 / ERTD_F64):
 * t = X[i, f] - min_[f]; out[i, f] = t / scale[f].  Both operations are
 * float64; for a float32 array t and the quotient are each rounded to
 * float32 (sklearn applies -= and /= in place to the float32 array).  out
 * (row pitch ldo, X's dtype) may be X.                                      */
int ertd_minmax_inverse(const void* X, int dtype, long long n, long long F, long long ldx,
                        const double* scale, const double* min_, void* out, long long ldo,
                        void* stream);
/* Scale, transpose and narrow in one pass (:259-261, :72, .float()):
 * X (n, L, C) float64 contiguous, scale / min_ (L * C) ->
 *   cond[i, c, l] = (float)(X[i, l, c] * scale[l C + c] + min_[l C + c])
 * cond (n, C, L) float32 contiguous: the product and the sum are rounded to
 * float64, then one round-to-nearest-even narrowing.  1 <= C <= 16; C = 14
 * with a 16-byte aligned X is the tuned path.  To fill rows
 * r0.. of a larger (N, C, L) buffer pass cond + r0 * C * L.                 */
int ertd_minmax_cond(const double* X, long long n, int L, int C, const double* scale,
                     const double* min_, float* cond, void* stream);
/* The way back (:417-419): cond (n, C, L) float32 -> out (n, L, C) float32,
 *   t = (float)(cond[i, c, l] - min_[l C + c]); out[i, l, c] = (float)(t / scale[l C + c])
 * with float64 operations, as ertd_minmax_inverse does for a float32 array. */
int ertd_minmax_cond_inverse(const float* cond, long long n, int L, int C, const double* scale,
                             const double* min_, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ERTDIFF_H */
