/*
 * ngp_hip.h — C ABI of the MI355X (gfx950) instant-ngp hot path.
 *
 * One shared library (libngp_hip.so) exports every entry point below. The
 * signatures take plain device pointers, sizes and a hipStream_t (passed as
 * void*), never torch types, so any host language can bind them (ctypes,
 * cgo, JNI, N-API). Each entry replaces one pybind11 function of the reference
 * extension; the reference declaration it stands in for is cited per function
 * (paths relative to the reference repository root).
 *
 * Conventions shared by every function:
 *   - The caller allocates every output and scratch buffer; nothing here calls
 *     hipMalloc/hipFree or synchronises, so each call can be captured into a
 *     hipGraph. Work is enqueued on `stream` (NULL = the legacy null stream).
 *   - Return value: NGP_OK (0) on success, a negative NGP_ERR_* code otherwise.
 *     NGP_ERR_ARG / NGP_ERR_UNSUPPORTED mirror the reference's TORCH_CHECK /
 *     std::runtime_error("... must be ...") failures; the Python shims raise
 *     RuntimeError with the reference's wording.
 *   - dtype codes: NGP_DTYPE_F32 = 0, NGP_DTYPE_F16 = 1, NGP_DTYPE_F64 = 2;
 *     NGP_DTYPE_U8 = 3 (the image source's pixels only).
 */
#ifndef NGP_HIP_H
#define NGP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NGP_OK 0
#define NGP_ERR_ARG (-1)
#define NGP_ERR_HIP (-2)
#define NGP_ERR_UNSUPPORTED (-3)

#define NGP_DTYPE_F32 0
#define NGP_DTYPE_F16 1
#define NGP_DTYPE_F64 2
#define NGP_DTYPE_U8 3

/* Library identification: ABI version (bumped on any signature change). */
int ngp_abi_version(void);
/* Human-readable message for the last NGP_ERR_* returned on this thread. */
const char* ngp_last_error(void);

/* ------------------------------------------------------------------------ */
/* gridencoder                                                              */
/* ------------------------------------------------------------------------ */

/* Replaces grid_encode_forward, gridencoder/src/gridencoder.h:12 and
 * gridencoder/src/gridencoder.cu:445-468.
 *   inputs  f32 [B, D] in [0,1]; embeddings dtype [sum_T, C];
 *   offsets i32 [L+1] (device); dy_dx dtype [B, L*D*C] or NULL.
 *   out_layout 0: outputs [L, B, C] (the reference layout);
 *   out_layout 1: outputs [B, L*C] (the layout the MLP consumes, no permute).
 *   D in {2,3,4,5}, C in {1,2,4,8}, L <= 64. */
int ngp_grid_encode_forward(const float* inputs, const void* embeddings, const int32_t* offsets,
                            void* outputs, uint32_t B, uint32_t D, uint32_t C, uint32_t L,
                            float S, uint32_t H, void* dy_dx, uint32_t gridtype,
                            int32_t align_corners, uint32_t interp, int32_t dtype,
                            int32_t out_layout, void* stream);

/* Replaces grid_encode_backward, gridencoder/src/gridencoder.h:13 and
 * gridencoder/src/gridencoder.cu:470-500. grad_embeddings must be zeroed by
 * the caller (scatter-add target). grad_layout as out_layout above. */
int ngp_grid_encode_backward(const void* grad, const float* inputs, const void* embeddings,
                             const int32_t* offsets, void* grad_embeddings, uint32_t B, uint32_t D,
                             uint32_t C, uint32_t L, float S, uint32_t H, const void* dy_dx,
                             void* grad_inputs, uint32_t gridtype, int32_t align_corners,
                             uint32_t interp, int32_t dtype, int32_t grad_layout, void* stream);

/* Replaces grad_total_variation, gridencoder/src/gridencoder.h:15 and
 * gridencoder/src/gridencoder.cu:636-642 (inputs are dtype, like the reference). */
int ngp_grad_total_variation(const void* inputs, const void* embeddings, void* grad,
                             const int32_t* offsets, float weight, uint32_t B, uint32_t D,
                             uint32_t C, uint32_t L, float S, uint32_t H, uint32_t gridtype,
                             int32_t align_corners, int32_t dtype, void* stream);

/* ------------------------------------------------------------------------ */
/* raymarching (all float32, like the reference wrappers' cast_inputs)      */
/* ------------------------------------------------------------------------ */

/* raymarching/src/raymarching.h:7, raymarching.cu:148-156 */
int ngp_near_far_from_aabb(const float* rays_o, const float* rays_d, const float* aabb, uint32_t N,
                           float min_near, float* nears, float* fars, void* stream);
/* raymarching.h:8, raymarching.cu:201-209 */
int ngp_sph_from_ray(const float* rays_o, const float* rays_d, float radius, uint32_t N,
                     float* coords, void* stream);
/* raymarching.h:9, raymarching.cu:229-232 */
int ngp_morton3D(const int32_t* coords, uint32_t N, int32_t* indices, void* stream);
/* raymarching.h:10, raymarching.cu:257-260 */
int ngp_morton3D_invert(const int32_t* indices, uint32_t N, int32_t* coords, void* stream);
/* raymarching.h:11, raymarching.cu:292-300 */
int ngp_packbits(const float* grid, uint32_t N, float density_thresh, uint8_t* bitfield,
                 void* stream);

/* Replaces march_rays_train, raymarching.h:13 and raymarching.cu:311-492.
 * Offsets are a deterministic exclusive prefix sum in ray order (a valid
 * execution of the reference's atomicAdd ordering): rays[i] = (i, off_i, n_i).
 * counter[0] += total samples, counter[1] += N (same as the reference).
 * Samples of rays with off_i + n_i > M are dropped (reference :416); the
 * caller zero-fills xyzs/dirs/deltas like the reference wrapper does.
 * workspace: 16-byte aligned device scratch of at least
 * ngp_march_rays_train_workspace_bytes (one float per possible sample,
 * N * max_steps, plus an occupancy image of ~C * H^3 / 6 bytes), e.g. from
 * the caller's caching allocator. */
size_t ngp_march_rays_train_workspace_bytes(uint32_t N, uint32_t max_steps, uint32_t C, uint32_t H);
/* Byte offset, inside that workspace, of a u32 error word the fused march +
 * Adam launch's in-launch emit sets when one of its bounded cross-workgroup
 * waits ran out (bit 0: a lower block's sample total, bit 1: the block's own
 * offsets); the offsets it wrote are then wrong. Sticky; the caller reads and
 * clears it (FusedTrainer.device_errors). No reference counterpart: the
 * reference's march (raymarching.cu:405-406) takes its offsets with atomics. */
size_t ngp_march_rays_train_error_offset(uint32_t N, uint32_t max_steps, uint32_t C, uint32_t H);
int ngp_march_rays_train(const float* rays_o, const float* rays_d, const uint8_t* grid,
                         float bound, float dt_gamma, uint32_t max_steps, uint32_t N, uint32_t C,
                         uint32_t H, uint32_t M, const float* nears, const float* fars,
                         float* xyzs, float* dirs, float* deltas, int32_t* rays, int32_t* counter,
                         const float* noises, void* workspace, size_t workspace_bytes,
                         void* stream);

/* The occupancy image march_rays_train builds from `grid` on every call can be
 * built once per bitfield change instead: ngp_march_occupancy_build into the
 * workspace, then ngp_march_rays_train_prebuilt (same arguments) as long as
 * grid's contents are unchanged. */
int ngp_march_occupancy_build(const uint8_t* grid, uint32_t C, uint32_t H, uint32_t N,
                              uint32_t max_steps, void* workspace, size_t workspace_bytes,
                              void* stream);
int ngp_march_rays_train_prebuilt(const float* rays_o, const float* rays_d, const uint8_t* grid,
                                  float bound, float dt_gamma, uint32_t max_steps, uint32_t N,
                                  uint32_t C, uint32_t H, uint32_t M, const float* nears,
                                  const float* fars, float* xyzs, float* dirs, float* deltas,
                                  int32_t* rays, int32_t* counter, const float* noises,
                                  void* workspace, size_t workspace_bytes, void* stream);
/* ngp_march_rays_train_prebuilt plus the tail of a fused step whose optimizer
 * update was launched by ngp_fused_optimizer_update_head: the deferred
 * GradScaler / LR / loss bookkeeping (scaler arguments as
 * ngp_fused_optimizer_step; loss_ray: the previous batch's N per-ray losses)
 * and ngp_ffmlp_pack of n_nets networks, as an extra row of blocks of the
 * emit launch. */
int ngp_march_rays_train_prebuilt_tail(const float* rays_o, const float* rays_d, const uint8_t* grid,
                                       float bound, float dt_gamma, uint32_t max_steps, uint32_t N,
                                       uint32_t C, uint32_t H, uint32_t M, const float* nears,
                                       const float* fars, float* xyzs, float* dirs, float* deltas,
                                       int32_t* rays, int32_t* counter, const float* noises,
                                       void* workspace, size_t workspace_bytes, void* state,
                                       float growth_factor, float backoff_factor, int32_t growth_interval,
                                       int32_t scaler_enabled, const float* loss_ray, int32_t n_nets,
                                       const void* const* mlp_weights, const uint32_t* in_dims,
                                       const uint32_t* hidden_dims, const uint32_t* num_layers,
                                       void* const* images, void* stream);

/* ngp_march_rays_train_prebuilt_tail whose march launch also carries a
 * deferred optimizer update (world 1, fused step): the march's workgroups
 * split into march waves and Adam waves that sweep the parameters while the
 * march waves probe the occupancy image (a latency-bound LDS chain beside an
 * HBM stream). job: ngp_fused_optimizer_update's arguments; its scaler check
 * must already be done (NGP_SCALER_PRECHECKED: the backward's kernels set the
 * found-inf flag). The batch must come from ngp_fused_step_head (n_nets 0);
 * the deferred bookkeeping and the MLP packs stay in the emit launch. */
#define NGP_ADAM_JOB_MAX_TENSORS 8
typedef struct ngp_adam_job {
    int32_t n_tensors;
    float* params[NGP_ADAM_JOB_MAX_TENSORS];
    void* grads[NGP_ADAM_JOB_MAX_TENSORS];       /* fp16 */
    float* exp_avg[NGP_ADAM_JOB_MAX_TENSORS];
    float* exp_avg_sq[NGP_ADAM_JOB_MAX_TENSORS];
    void* half_params[NGP_ADAM_JOB_MAX_TENSORS]; /* fp16 shadows or NULL */
    uint64_t sizes[NGP_ADAM_JOB_MAX_TENSORS];
    float lr, beta1, beta2, eps;
    int32_t iters, zero_grads;
    float grad_mult;
    void* clear;            /* zeroed by the launch too (the grid backward's bin cursors), or NULL */
    uint32_t clear_bytes;   /* multiple of 16, clear 16-byte aligned */
    uint32_t flags;         /* NGP_ADAM_JOB_TAIL_LATER | NGP_ADAM_JOB_EMIT_LAUNCH (below) or 0 */
} ngp_adam_job;
/* ... and the emit launch's whole tail row (bookkeeping + MLP fragment packs) is
 * left to ngp_grid_encode_forward_fused_tail: with the samples emitted by the
 * march launch itself, the march is then ONE launch */
#define NGP_ADAM_JOB_TAIL_LATER 2u
/* ... and the samples are emitted by the march's own emit launch instead of
 * inside the march + Adam launch (the in-launch emit's equivalence tests) */
#define NGP_ADAM_JOB_EMIT_LAUNCH 4u
int ngp_march_rays_train_prebuilt_adam(const float* rays_o, const float* rays_d, const uint8_t* grid,
                                       float bound, float dt_gamma, uint32_t max_steps, uint32_t N,
                                       uint32_t C, uint32_t H, uint32_t M, const float* nears,
                                       const float* fars, float* xyzs, float* dirs, float* deltas,
                                       int32_t* rays, int32_t* counter, const float* noises,
                                       void* workspace, size_t workspace_bytes, void* state,
                                       float growth_factor, float backoff_factor, int32_t growth_interval,
                                       int32_t scaler_enabled, const float* loss_ray, int32_t n_nets,
                                       const void* const* mlp_weights, const uint32_t* in_dims,
                                       const uint32_t* hidden_dims, const uint32_t* num_layers,
                                       void* const* images, const ngp_adam_job* job, void* stream);

/* raymarching.h:14, raymarching.cu:580-588 */
int ngp_composite_rays_train_forward(const float* sigmas, const float* rgbs, const float* deltas,
                                     const int32_t* rays, uint32_t M, uint32_t N, float T_thresh,
                                     float* weights_sum, float* depth, float* image, void* stream);
/* raymarching.h:15, raymarching.cu:694-702. grad_sigmas / grad_rgbs are
 * zeroed by the caller (entries past a ray's early stop are not written). */
int ngp_composite_rays_train_backward(const float* grad_weights_sum, const float* grad_depth,
                                      const float* grad_image, const float* sigmas,
                                      const float* rgbs, const float* deltas, const int32_t* rays,
                                      const float* weights_sum, const float* depth,
                                      const float* image, uint32_t M, uint32_t N, float T_thresh,
                                      float* grad_sigmas, float* grad_rgbs, void* stream);
/* The distortion regulariser (the reference's loss.py EffDistLoss) on the
 * training composite's weights, serial per ray with the composite's
 * T *= 1 - alpha recurrence and stop rule:
 *   dist[ray index] = sum_ij w_i w_j |m_i - m_j| + 1/3 sum_i deltas[i][0] w_i^2
 * (m the running sum of deltas[.][1]; 0 for a ray without samples or dropped
 * for overflowing M). The backward writes grad_dist[ray] * d dist / d sigma for
 * the samples up to the stop; the caller zeroes grad_sigmas [M]. */
int ngp_distortion_rays_train_forward(const float* sigmas, const float* deltas, const int32_t* rays,
                                      uint32_t M, uint32_t N, float T_thresh, float* dist, void* stream);
int ngp_distortion_rays_train_backward(const float* grad_dist, const float* sigmas, const float* deltas,
                                       const int32_t* rays, const float* dist, uint32_t M, uint32_t N,
                                       float T_thresh, float* grad_sigmas, void* stream);
/* raymarching.h:17, raymarching.cu:817-825 */
int ngp_march_rays(uint32_t n_alive, uint32_t n_step, const int32_t* rays_alive,
                   const float* rays_t, const float* rays_o, const float* rays_d, float bound,
                   float dt_gamma, uint32_t max_steps, uint32_t C, uint32_t H, const uint8_t* grid,
                   const float* nears, const float* fars, float* xyzs, float* dirs, float* deltas,
                   const float* noises, void* stream);
/* raymarching.h:18, raymarching.cu:917-923 (in place; rays_alive[n] = -1 on termination) */
int ngp_composite_rays(uint32_t n_alive, uint32_t n_step, float T_thresh, int32_t* rays_alive,
                       float* rays_t, const float* sigmas, const float* rgbs, const float* deltas,
                       float* weights_sum, float* depth, float* image, void* stream);

/* Device-driven inference render loop (the alive-ray loop of run_cuda with
 * training off, renderer.py:376-426, without its host round trip per
 * iteration). The loop state is a two-slot device record (state_bytes);
 * iteration i reads slot i & 1 and prepares slot (i + 1) & 1:
 *   render_init: alive list 0 = arange(N), rays_t = nears, outputs zeroed;
 *   render_march: kernel_march_rays (raymarching.cu:709-814) for the
 *     iteration's n_alive and n_step = max(min(N / n_alive, 8), 1), unused
 *     sample slots zeroed, noise in the first iteration only; writes the
 *     iteration's sample count (render_count) for the grid / MLP kernels;
 *   render_composite: kernel_composite_rays (raymarching.cu:827-914) on
 *     sigmas [n_alive * n_step] and the colour network's fp16 logits
 *     color_out [*, 16] (rgb = half(sigmoid)), appending surviving rays to
 *     rays_alive_next (order within the list is unspecified; per-ray results
 *     do not depend on it).
 * Once step >= max_steps or no ray is alive, every launch is a no-op. */
size_t ngp_render_state_bytes(void);
int32_t* ngp_render_count(void* state, uint32_t iter);
int ngp_render_init(uint32_t N, const float* nears, int32_t* rays_alive, float* rays_t, float* weights_sum,
                    float* depth, float* image, void* state, void* stream);
int ngp_render_march(uint32_t N, uint32_t iter, void* state, const int32_t* rays_alive, const float* rays_t,
                     const float* rays_o, const float* rays_d, float bound, float dt_gamma, uint32_t max_steps,
                     uint32_t C, uint32_t H, const uint8_t* grid, const float* fars, float* xyzs, float* dirs,
                     float* deltas, const float* noises, void* stream);
int ngp_render_composite(uint32_t N, uint32_t iter, uint32_t max_steps, void* state, float T_thresh,
                         const int32_t* rays_alive, int32_t* rays_alive_next, float* rays_t, const float* sigmas,
                         const void* color_out, const float* deltas, float* weights_sum, float* depth,
                         float* image, void* stream);

/* ------------------------------------------------------------------------ */
/* shencoder                                                                */
/* ------------------------------------------------------------------------ */

/* shencoder/src/shencoder.h:9, shencoder.cu:420-439. dtype F32 or F64.
 * C is the degree (1..8), outputs [B, C*C]; dy_dx [B, D*C*C] or NULL. */
int ngp_sh_encode_forward(const void* inputs, void* outputs, uint32_t B, uint32_t D, uint32_t C,
                          void* dy_dx, int32_t dtype, void* stream);
/* shencoder.h:10, shencoder.cu:441-454. grad_inputs zeroed by the caller. */
int ngp_sh_encode_backward(const void* grad, const void* inputs, uint32_t B, uint32_t D,
                           uint32_t C, const void* dy_dx, void* grad_inputs, int32_t dtype,
                           void* stream);

/* ------------------------------------------------------------------------ */
/* freqencoder                                                              */
/* ------------------------------------------------------------------------ */

/* freqencoder/src/freqencoder.h:7, freqencoder.cu:97-111
 * (kernel_freq :30-59). inputs f32 [B, D], outputs f32 [B, C] with
 * C = D (1 + 2 deg): [x, sin(2^0 x), cos(2^0 x), ..., cos(2^(deg-1) x)]. */
int ngp_freq_encode_forward(const float* inputs, uint32_t B, uint32_t D, uint32_t deg, uint32_t C,
                            float* outputs, void* stream);
/* freqencoder.h:10, freqencoder.cu:114-131 (kernel_freq_backward :63-94). grad f32 [B, C],
 * outputs the forward's; grad_inputs f32 [B, D] is written (not added to). */
int ngp_freq_encode_backward(const float* grad, const float* outputs, uint32_t B, uint32_t D,
                             uint32_t deg, uint32_t C, float* grad_inputs, void* stream);

/* ------------------------------------------------------------------------ */
/* ffmlp (fp16 storage, fp16 MFMA with fp32 accumulation)                   */
/* ------------------------------------------------------------------------ */

/* ffmlp/src/ffmlp.h:8, ffmlp.cu:635-671. inputs f16 [B, input_dim], weights
 * f16 flat (per layer row-major [out, in], nn.Linear layout), outputs f16
 * [B, output_dim]. forward_buffer f16 [num_layers, B, hidden] or NULL (the
 * backward below recomputes activations and never reads it).
 * Supported on this build: hidden_dim in {32, 64}, input_dim % 16 == 0 and
 * <= 64, output_dim == 16 (FFMLP pads outputs to 16), num_layers 2..4, any B.
 * Other shapes return NGP_ERR_UNSUPPORTED with the reason in ngp_last_error. */
int ngp_ffmlp_forward(const void* inputs, const void* weights, uint32_t B, uint32_t input_dim,
                      uint32_t output_dim, uint32_t hidden_dim, uint32_t num_layers,
                      uint32_t activation, uint32_t output_activation, void* forward_buffer,
                      void* outputs, void* stream);
/* ffmlp.h:9, ffmlp.cu:673-709 */
int ngp_ffmlp_inference(const void* inputs, const void* weights, uint32_t B, uint32_t input_dim,
                        uint32_t output_dim, uint32_t hidden_dim, uint32_t num_layers,
                        uint32_t activation, uint32_t output_activation, void* inference_buffer,
                        void* outputs, void* stream);
/* Workspace (bytes) ngp_ffmlp_backward needs for its per-workgroup dW slabs. */
size_t ngp_ffmlp_backward_workspace_bytes(uint32_t B, uint32_t input_dim, uint32_t output_dim,
                                          uint32_t hidden_dim, uint32_t num_layers);
/* ffmlp.h:11, ffmlp.cu:749-895. grad f16 [B, output_dim]; grad_inputs f16
 * [B, input_dim] (written when calc_grad_inputs); grad_weights flat, dtype
 * gw_dtype (F16 like the reference, or F32), overwritten (not accumulated).
 * forward_buffer / backward_buffer may be NULL. */
int ngp_ffmlp_backward(const void* grad, const void* inputs, const void* weights,
                       const void* forward_buffer, uint32_t B, uint32_t input_dim,
                       uint32_t output_dim, uint32_t hidden_dim, uint32_t num_layers,
                       uint32_t activation, uint32_t output_activation, int32_t calc_grad_inputs,
                       void* backward_buffer, void* grad_inputs, void* grad_weights,
                       int32_t gw_dtype, void* workspace, size_t workspace_bytes, void* stream);
/* ffmlp.h:12-13, ffmlp.cu:711-740. The side-stream split-K pool of the
 * reference is not needed (dW is reduced in-kernel); kept as no-ops so the
 * FFMLP module's construction sequence is unchanged. */
int ngp_ffmlp_allocate_splitk(size_t size);
int ngp_ffmlp_free_splitk(void);

/* ------------------------------------------------------------------------ */
/* optimizer (next row of SURVEY §8f): fused Adam over a flat f32 param set */
/* ------------------------------------------------------------------------ */

/* torch.optim.Adam semantics (main_nerf.py:194; betas (0.9,0.99), eps 1e-15):
 * m = b1*m + (1-b1)*g; v = b2*v + (1-b2)*g*g;
 * p -= lr/bc1 * m / (sqrt(v)/sqrt(bc2) + eps), g = grad (f32 or f16) * grad_scale.
 * step is the 1-based step count after increment. */
int ngp_adam_step(float* params, const void* grads, int32_t grad_dtype, float* exp_avg,
                  float* exp_avg_sq, size_t n, float lr, float beta1, float beta2, float eps,
                  float weight_decay, int32_t step, float grad_scale, void* stream);

/* Exponential moving average of a flat parameter vector, torch_ema's
 * ExponentialMovingAverage.update() in one pass:
 *   shadow[i] = shadow[i] - one_minus_decay * (shadow[i] - param[i])
 * in fp32, in exactly that order (tmp = s - p; tmp *= 1 - decay; s -= tmp),
 * without contraction: torch's three operations bit for bit. 16-byte accesses
 * in a grid-stride loop, the last n % 4 elements one by one; 12 B per
 * parameter. n == 0: nothing is launched, NGP_OK. Null or not 16-byte aligned
 * pointers: NGP_ERR_ARG. */
int ngp_ema_update(float* shadow, const float* param, uint64_t n, float one_minus_decay, void* stream);

/* ---------------------------------------------------------------------------
 * Fused train step (DESIGN.md "fused step"). No reference counterpart as C
 * functions: together they replace the elementwise torch glue of one
 * reference training iteration (nerf/utils.py train_step :453-497 with
 * GradScaler/Adam :194-217, renderer.run_cuda :257-375, network_ff.forward
 * :69-105, gridencoder/grid.py:61-89 casts) with fused kernels. `count`
 * arguments are device pointers to the marcher's sample count: rows at or
 * past it are not computed. `state` is a device StepState
 * (ngp_fused_state_bytes). */
/* embeddings: the fp32 table (emb_dtype NGP_DTYPE_F32, rounded to half on
 * load) or its fp16 copy (NGP_DTYPE_F16, e.g. the one the fused optimizer
 * refreshes after every update): identical results, half the gather bytes. */
int ngp_grid_encode_forward_fused(const float* xyz, float bound, const void* embeddings,
                                  int32_t emb_dtype, const int32_t* offsets, void* outputs, uint32_t B,
                                  const int32_t* count, uint32_t D, uint32_t C, uint32_t L, float S,
                                  uint32_t H, uint32_t gridtype, int32_t align_corners,
                                  uint32_t interp, int32_t out_layout, void* stream);
/* Binned backward (hashed levels without scattered atomics) when workspace is
 * given: offsets_host is a host copy of offsets; the workspace (size from
 * ngp_grid_encode_backward_fused_workspace_bytes, 0 if nothing is binned) must
 * be zero-filled before its first use and is left ready for the next call.
 * nonfinite (nullable; needs offsets_host): set to 1 when a grad entry this
 * call leaves in grad_embeddings is inf/nan: GradScaler's check (torch
 * amp _amp_foreach_non_finite_check_and_unscale_) made by the kernels that
 * write the values (binned levels) or a scan of the other levels. */
size_t ngp_grid_encode_backward_fused_workspace_bytes(uint32_t B, uint32_t D, uint32_t C, uint32_t L,
                                                      float S, uint32_t H, int32_t align_corners,
                                                      const int32_t* offsets_host);
/* grad_layout | NGP_GRID_GRAD_ZEROED: grad_embeddings is all zeros on entry
 * (the fused optimizer clears it), so bins that own their table slice store
 * their sums instead of reading the slice back first. */
#define NGP_GRID_GRAD_ZEROED 0x10
/* grad_layout | NGP_GRID_CURSORS_EXTERNAL: the caller zeroes the workspace's
 * first ngp_grid_encode_backward_fused_counter_bytes bytes (the bin cursors and
 * the 512-byte area after them) between calls (the fused step's march launch
 * does), so the call does not leave them zeroed itself. With
 * NGP_GRID_GRAD_ZEROED too, the hashed levels' bins are summed one per wave
 * (same sums, same bits as the workgroup image path; round 7). */
#define NGP_GRID_CURSORS_EXTERNAL 0x20
/* grad_layout | NGP_GRID_TIMING: the binned launches time themselves on the
 * chip's 100 MHz constant clock (s_memrealtime) into a ring in the workspace
 * (ngp_grid_encode_backward_fused_timing_offset; u32 words): [0] calls so
 * far; the head of call c at word 64 + 4 (c % NGP_GRID_TIMING_RING) holds
 * {start (bin launch, block (0, 0)), samples, accumulate workgroups n, 0};
 * its ends at word 64 + 4 NGP_GRID_TIMING_RING + (c % RING) MAX_WG + w, one
 * per accumulate workgroup w < n. A call's span is max_w(end_w - start)
 * (mod 2^32 ticks of 10 ns). Plain stores only: the timed kernels keep their
 * critical path. Zero word 0 to restart. */
#define NGP_GRID_TIMING 0x40
#define NGP_GRID_TIMING_RING 256
#define NGP_GRID_TIMING_MAX_WG 1024
size_t ngp_grid_encode_backward_fused_timing_offset(uint32_t B, uint32_t D, uint32_t C, uint32_t L, float S,
                                                    uint32_t H, int32_t align_corners, const int32_t* offsets_host);
size_t ngp_grid_encode_backward_fused_counter_bytes(uint32_t B, uint32_t D, uint32_t C, uint32_t L, float S,
                                                    uint32_t H, int32_t align_corners,
                                                    const int32_t* offsets_host);
int ngp_grid_encode_backward_fused(const void* grad, const float* xyz, float bound,
                                   const int32_t* offsets, void* grad_embeddings, uint32_t B,
                                   const int32_t* count, uint32_t D, uint32_t C, uint32_t L, float S,
                                   uint32_t H, uint32_t gridtype, int32_t align_corners,
                                   uint32_t interp, const int32_t* offsets_host, void* workspace,
                                   size_t workspace_bytes, int32_t grad_layout, int32_t* nonfinite,
                                   void* stream);
/* ngp_grid_encode_backward_fused plus ngp_ffmlp_reduce of n_nets deferred MLP
 * backward calls (its arguments, fp16 grad_weights, mlp_nonfinite as its
 * nonfinite) carried by the bin launch as an extra column of blocks: the same
 * sums in the same order, one launch less. Without binned levels the reduce
 * runs on its own first. */
int ngp_grid_encode_backward_fused_reduce(const void* grad, const float* xyz, float bound, const int32_t* offsets,
                                          void* grad_embeddings, uint32_t B, const int32_t* count, uint32_t D,
                                          uint32_t C, uint32_t L, float S, uint32_t H, uint32_t gridtype,
                                          int32_t align_corners, uint32_t interp, const int32_t* offsets_host,
                                          void* workspace, size_t workspace_bytes, int32_t grad_layout,
                                          int32_t* nonfinite, int32_t n_nets, void* const* mlp_workspaces,
                                          const uint32_t* mlp_Bs, const uint32_t* in_dims,
                                          const uint32_t* hidden_dims, const uint32_t* num_layers,
                                          void* const* grad_weights, int32_t* mlp_nonfinite, void* stream);
/* The fused step's next batch (ngp_fused_step_head's sampler arguments),
 * drawn by ngp_grid_encode_backward_fused_reduce_batch while this batch's
 * backward runs: the batch buffers are dead once the composite has read its
 * targets. The draw records this batch's counts (step_counter) without
 * resetting the counter, which the backward still reads; the accumulate
 * resets it. */
typedef struct ngp_batch_job {
    const float* poses;
    uint32_t n_poses;
    const float* intrinsics4;
    uint32_t H, W, N;
    const float* boxes;
    int32_t nboxes;
    const float* aabb6;
    float min_near;
    uint32_t seed;
    void* state;
    float *rays_o, *rays_d, *rgba, *bg, *nears, *fars, *noises;
    int32_t *counter, *step_counter;
} ngp_batch_job;
/* ngp_grid_encode_backward_fused_reduce + the next batch (job) as another
 * column of blocks of the bin launch. Requires a binned plan. */
int ngp_grid_encode_backward_fused_reduce_batch(const void* grad, const float* xyz, float bound,
                                                const int32_t* offsets, void* grad_embeddings, uint32_t B,
                                                const int32_t* count, uint32_t D, uint32_t C, uint32_t L,
                                                float S, uint32_t H, uint32_t gridtype, int32_t align_corners,
                                                uint32_t interp, const int32_t* offsets_host, void* workspace,
                                                size_t workspace_bytes, int32_t grad_layout, int32_t* nonfinite,
                                                int32_t n_nets, void* const* mlp_workspaces, const uint32_t* mlp_Bs,
                                                const uint32_t* in_dims, const uint32_t* hidden_dims,
                                                const uint32_t* num_layers, void* const* grad_weights,
                                                int32_t* mlp_nonfinite, const ngp_batch_job* job, void* stream);
/* ngp_grid_encode_backward_fused_reduce_batch over the rows live_rows[0 ..
 * *live_count) (the sample rows of xyz and of the [L, B, C] grad). */
int ngp_grid_encode_backward_fused_reduce_batch_live(
    const void* grad, const float* xyz, float bound, const int32_t* offsets, void* grad_embeddings, uint32_t B,
    const int32_t* live_rows, const int32_t* live_count, uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H,
    uint32_t gridtype, int32_t align_corners, uint32_t interp, const int32_t* offsets_host, void* workspace,
    size_t workspace_bytes, int32_t grad_layout, int32_t* nonfinite, int32_t n_nets, void* const* mlp_workspaces,
    const uint32_t* mlp_Bs, const uint32_t* in_dims, const uint32_t* hidden_dims, const uint32_t* num_layers,
    void* const* grad_weights, int32_t* mlp_nonfinite, const ngp_batch_job* job, void* stream);
/* The fused step's batch drawn from an image dataset instead of the analytic
 * boxes (the reference's training collate, nerf/provider.py:442-508, with
 * preloaded images): ray n of a draw takes its RGBA target from
 * pixels[pose][pix], everything else (pose, pixel, ray, background, march
 * noise, near/far, the counter bookkeeping) as ngp_lego_rays draws it from the
 * same counter-RNG streams, so the same seed, poses and intrinsics give the
 * same rays bit for bit.
 *   pixels: [n_poses, H, W, channels], dtype NGP_DTYPE_U8 (converted as
 *     (float)v / 255.0f, a true division) or NGP_DTYPE_F32; RGBA pixels are
 *     one load each, so 4-byte (uint8) / 16-byte (float32) aligned.
 *   channels 4: RGBA target, random background (as ngp_lego_rays);
 *   channels 3: target (r, g, b, 1) and background (1, 1, 1): the reference's
 *     bg_color = 1 for 3-channel images (nerf/utils.py:508-509); the loss's
 *     blend rgb * 1 + 1 * 0 then reproduces gt_rgb = images exactly.
 *   pix (nullable) i32 [N]: each ray's flat pixel index j * W + i (the
 *     reference's results['inds'], nerf/utils.py:112);
 *   image_index (nullable) i32 [1]: the draw's image.
 *   depths (nullable) f32 [n_poses, H, W]: a depth map per image (the
 *     reference's dep_path maps, nerf/provider.py:346-357, 555-557). Ray n then
 *     also gets depth_out[n] = depths[pose][pix] * depth_scale (one fp32
 *     multiply: file units -> ngp units), from the pose and pixel its colour
 *     comes from. Null (a zeroed tail): colours only, as before these fields.
 *   depth_out f32 [N]: required with depths.
 *   error_map (nullable) f32 [n_poses, res * res]: the reference's --error_map
 *     (nerf/provider.py:397-401, nerf/utils.py:101-113): a coarse res x res
 *     error image per pose, cell = row_cell * res + col_cell, finite and >= 0.
 *     The draw's pixels then come from the N cells ngp_error_map_select chose
 *     for this draw (`selected`, ascending), not from stream 1's uniform pixel:
 *       r    = rng_u32(seed, it, 0xffffffff, 1) % N
 *       cell = selected[((uint64)n * perm_mult + r) % N]
 *       sx = (float)H / res, sy = (float)W / res           (fp32, no contraction)
 *       row = min((uint32)((float)(cell / res) * sx + rng_unit(seed, it, n, 7) * sx), H - 1)
 *       col = min((uint32)((float)(cell % res) * sy + rng_unit(seed, it, n, 8) * sy), W - 1)
 *       pix = row * W + col, coarse[n] = cell
 *     and everything else of ray n (direction from pix, target and depth
 *     gather, background, noise, near/far, counters) is unchanged. Null (a
 *     zeroed tail): the uniform draw, bit for bit as before these fields.
 *   error_map_res: 1..128 with a map.
 *   selected i32 [N]: ngp_error_map_select's output for this draw; the select
 *     is issued on the same stream just before the launch that draws.
 *   perm_mult: in [1, N], coprime to N, so that n -> (n * perm_mult + r) % N
 *     is a permutation (the caller's: the largest such integer <= 0.618 N
 *     spreads the ascending cells over the ray indices).
 *   coarse i32 [N] by ray index: the reference's inds_coarse, read back by
 *     ngp_error_map_update. Required with a map.
 * Bad channels / dtype / null pixels, depths without depth_out, a map without
 * selected / coarse or with a res outside 1..128, N > res * res or a
 * perm_mult that is no permutation of N, map fields without a map:
 * NGP_ERR_ARG before any device work. */
typedef struct ngp_image_source {
    const void* pixels;
    uint32_t channels;
    int32_t dtype;
    int32_t* pix;
    int32_t* image_index;
    const float* depths;
    float depth_scale;
    float* depth_out;
    const float* error_map;
    uint32_t error_map_res;
    const int32_t* selected;
    uint32_t perm_mult;
    int32_t* coarse;
} ngp_image_source;
/* Weighted draw without replacement of N of the res * res cells of one row of
 * the error map, torch.multinomial(w, N, replacement=False)'s exponential race
 * on the counter RNG (nerf/utils.py:104): with it = state->draw (the draw the
 * next batch launch makes) and pose = rng_u32(seed, it, 0xffffffff, 0) % n_poses,
 * cell c of row `pose` (weight w) gets
 *   k = rng_u32(seed, it, c, 6) >> 8,  u = (float)(k + 1) * 2^-24  in (0, 1]
 *   key = w > 0 ? w / -logf(u) : 0           (u = 1: +inf)
 * and the N largest keys win, ties (the all-zero map too) to the lower cell.
 * selected[N]: the winners in ascending cell order, the same bytes on every
 * run. keys_out (nullable) f32 [res * res]: every cell's key. One workgroup;
 * nothing is read back to the host, so the launch replays in a graph.
 * Null map / selected / state, n_poses 0, res outside 1..128, N == 0 or
 * N > res * res: NGP_ERR_ARG before any device work. */
int ngp_error_map_select(const float* error_map, uint32_t n_poses, uint32_t res, uint32_t N, uint32_t seed,
                         const void* state, int32_t* selected, float* keys_out, void* stream);
/* The EMA the reference folds each ray's loss into the map with
 * (nerf/utils.py:578-600): for every ray n of the batch (rays without samples
 * or dropped past the sample budget too), with index = rays[n * 3],
 *   err = ((e0^2 + e1^2) + e2^2) * (1/3)f    the composite's per-ray colour term:
 *         e = out_image[index] - blend(gt[index], bg[index]), as
 *         ngp_nerf_composite_loss computes its loss_ray, whatever the weights
 *   map[image_index[0]][coarse[index]] = 0.1f * old + 0.9f * err
 * One deviation from the reference: a non-finite or negative err leaves the
 * cell as it was, so the map stays finite and >= 0 (the select relies on it).
 * out_image f32 [N, 3] by ray index is the composite's output of this batch;
 * gt f32 [N, gt_channels] and bg f32 [N, 3] are its targets. Cells are unique
 * within a batch (no race). Null buffers, n_poses 0, res outside 1..128,
 * N > res * res: NGP_ERR_ARG before any device work. */
int ngp_error_map_update(float* error_map, uint32_t n_poses, uint32_t res, uint32_t N, const int32_t* rays,
                         const float* out_image, const float* gt, uint32_t gt_channels, const float* bg,
                         const int32_t* image_index, const int32_t* coarse, void* stream);
/* ngp_lego_rays with the image source in place of the boxes. */
int ngp_image_rays(const float* poses, uint32_t n_poses, const float* intrinsics4, uint32_t H, uint32_t W,
                   uint32_t N, const ngp_image_source* src, const float* aabb6, float min_near, uint32_t seed,
                   void* state, float* rays_o, float* rays_d, float* rgba, float* bg, float* nears, float* fars,
                   float* noises, int32_t* counter, int32_t* step_counter, void* stream);
/* ngp_fused_step_head with the image source in place of the boxes. */
int ngp_fused_step_head_images(const float* poses, uint32_t n_poses, const float* intrinsics4, uint32_t H,
                               uint32_t W, uint32_t N, const ngp_image_source* src, const float* aabb6,
                               float min_near, uint32_t seed, void* state, float* rays_o, float* rays_d,
                               float* rgba, float* bg, float* nears, float* fars, float* noises, int32_t* counter,
                               int32_t* step_counter, float growth_factor, float backoff_factor,
                               int32_t growth_interval, int32_t scaler_enabled, const float* loss_ray,
                               int32_t n_nets, const void* const* mlp_weights, const uint32_t* in_dims,
                               const uint32_t* hidden_dims, const uint32_t* num_layers, void* const* images,
                               void* clear, uint32_t clear_bytes, void* stream);
/* ngp_grid_encode_backward_fused_reduce_batch_live whose next batch (job) is
 * drawn from the image source (job->boxes null, job->nboxes 0). live_rows
 * null: every row below *live_count, the marcher's sample count
 * (ngp_grid_encode_backward_fused_reduce_batch). */
int ngp_grid_encode_backward_fused_reduce_batch_images(
    const void* grad, const float* xyz, float bound, const int32_t* offsets, void* grad_embeddings, uint32_t B,
    const int32_t* live_rows, const int32_t* live_count, uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H,
    uint32_t gridtype, int32_t align_corners, uint32_t interp, const int32_t* offsets_host, void* workspace,
    size_t workspace_bytes, int32_t grad_layout, int32_t* nonfinite, int32_t n_nets, void* const* mlp_workspaces,
    const uint32_t* mlp_Bs, const uint32_t* in_dims, const uint32_t* hidden_dims, const uint32_t* num_layers,
    void* const* grad_weights, int32_t* mlp_nonfinite, const ngp_batch_job* job, const ngp_image_source* src,
    void* stream);
/* ngp_grid_encode_forward_fused (out_layout 0) with the fused step's tail as
 * extra workgroups dispatched first: the deferred GradScaler / LambdaLR / loss
 * bookkeeping of the update the march launch applied (state; when pending) and
 * the MLP fragment packs (ngp_ffmlp_pack's arguments; n_nets 0: none). For the
 * march launch of an ngp_adam_job with NGP_ADAM_JOB_TAIL_LATER. */
int ngp_grid_encode_forward_fused_tail(const float* xyz, float bound, const void* embeddings, int32_t emb_dtype,
                                       const int32_t* offsets, void* outputs, uint32_t B, const int32_t* count,
                                       uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H, uint32_t gridtype,
                                       int32_t align_corners, uint32_t interp, void* state, float growth_factor,
                                       float backoff_factor, int32_t growth_interval, int32_t scaler_enabled,
                                       const float* loss_ray, uint32_t n_rays, int32_t n_nets,
                                       const void* const* mlp_weights, const uint32_t* in_dims,
                                       const uint32_t* hidden_dims, const uint32_t* num_layers, void* const* images,
                                       void* stream);
/* Weight-fragment images (forward + transposed, per matmul) of n networks in
 * one launch; image k needs ngp_ffmlp_image_bytes of its network. The
 * forward/backward *_rows calls below take the image (nullable: the weights
 * are packed per call). */
size_t ngp_ffmlp_image_bytes(uint32_t in_dim, uint32_t hidden_dim, uint32_t num_layers);
int ngp_ffmlp_pack(int32_t n, const void* const* weights, const uint32_t* in_dims,
                   const uint32_t* hidden_dims, const uint32_t* num_layers, void* const* images,
                   void* stream);
int ngp_ffmlp_forward_rows(const void* inputs, const void* weights, const void* image, uint32_t B,
                           const int32_t* count, uint32_t in_dim, uint32_t output_dim,
                           uint32_t hidden_dim, uint32_t num_layers, uint32_t activation,
                           uint32_t output_activation, void* outputs, void* stream);
/* The NeRF sigma network with its glue as the epilogue (network_ff.py:61-68):
 * h_out [B,16] half, sigma [B] = density_scale * exp(h[:,0]) fp32, color_in
 * [B,32] half = [SH4(dirs) | h[:,1:16] | 0]. */
int ngp_nerf_sigma_forward(const void* inputs, const void* weights, const void* image, uint32_t B,
                           const int32_t* count, uint32_t in_dim, uint32_t hidden_dim,
                           uint32_t num_layers, void* h_out, float* sigma, void* color_in,
                           const float* dirs, float density_scale, uint32_t flags, void* stream);
/* The whole NeRF forward in one launch (network_ff.py:51-74): the sigma
 * network on pair-major encodings enc [16][B][2] (rows < *count), the
 * ngp_nerf_sigma_forward epilogue (h_out, sigma, color_in, same values), and
 * the colour network on color_in, rgb logits color_out [B,16] half. Images:
 * the two networks' ngp_ffmlp_pack images. 64-wide networks with 32 inputs,
 * num_layers 2..3 (sigma) and 2..4 (colour). No clamp in the forward: sigma is
 * inf where exp(h[:,0]) overflows fp32. All six depth pairs are held to the
 * float64 oracle and to the two launches in tests/test_gpu_nerf_net.py (cases
 * a, b); the default 2 / 3 also in tests/test_gpu_e2e_oracle.py. */
int ngp_nerf_forward(const void* enc, const void* sigma_image, const void* color_image, uint32_t B,
                     const int32_t* count, uint32_t hidden_dim, uint32_t num_layers,
                     uint32_t hidden_dim_color, uint32_t num_layers_color, void* h_out, float* sigma,
                     void* color_in, const float* dirs, float density_scale, void* color_out,
                     void* stream);
#define NGP_FFMLP_DEFER_REDUCE 1u /* leave dW partials for ngp_ffmlp_reduce */
#define NGP_FFMLP_NERF_GEO 2u     /* grad_inputs [B,16]: input-grad cols 16..30 -> cols 1..15 */
#define NGP_FFMLP_PAIR_MAJOR 4u   /* inputs and grad_inputs as [in_dim/2][B][2] (the grid's [L,B,2]) */
int ngp_ffmlp_backward_rows(const void* grad, const void* inputs, const void* weights,
                            const void* image, uint32_t B, const int32_t* count, uint32_t in_dim,
                            uint32_t output_dim, uint32_t hidden_dim, uint32_t num_layers,
                            uint32_t activation, void* grad_inputs, void* grad_weights,
                            int32_t gw_dtype, uint32_t flags, void* workspace,
                            size_t workspace_bytes, void* stream);
/* Fused-step: both FFMLP backwards of NeRFNetwork (nerf/network_ff.py:
 * color_net then sigma_net, each ffmlp.cu kernel_mlp_fused_backward :410-518)
 * in one launch. Equals ngp_ffmlp_backward_rows of the colour network
 * (flags NGP_FFMLP_NERF_GEO | NGP_FFMLP_DEFER_REDUCE, input width 32, writing
 * g_h[:, 1:16]) followed by that of the sigma network (grad g_h, inputs enc
 * [16][B][2], flags NGP_FFMLP_PAIR_MAJOR | NGP_FFMLP_DEFER_REDUCE, input
 * gradient g_enc): the input gradients bit for bit, the dW partials summed in
 * another order. Workspaces as ngp_ffmlp_backward_workspace_bytes of each
 * network; reduce with ngp_ffmlp_reduce. 64-wide networks, num_layers 2..3.
 * Rows at or past *count contribute nothing and keep their g_h / g_enc; with
 * *count <= 0 every workgroup still writes its (zero) dW partial. All four
 * depth pairs, here and in ngp_nerf_backward_live, are held to the float64
 * oracle and to the two calls in tests/test_gpu_nerf_net.py (cases c, d); the
 * default 2 / 3 also in tests/test_gpu_fused.py and tests/test_gpu_e2e_oracle.py.
 * timing (nullable): the grid backward's NGP_GRID_TIMING ring (the fused grid
 * workspace at ngp_grid_encode_backward_fused_timing_offset): workgroup b's
 * end goes into end slot NGP_GRID_TIMING_MAX_WG - 1 - b of the next call, and
 * the grid backward's span then starts at the latest of them. */
int ngp_nerf_backward(const void* g_color_out, const void* color_in, const void* color_image, void* g_h,
                      const void* enc, const void* sigma_image, void* g_enc, uint32_t B, const int32_t* count,
                      uint32_t hidden_dim, uint32_t num_layers, uint32_t hidden_dim_color,
                      uint32_t num_layers_color, void* sigma_workspace, size_t sigma_workspace_bytes,
                      void* color_workspace, size_t color_workspace_bytes, uint32_t* timing, void* stream);
/* ngp_nerf_backward over the rows live_rows[0 .. *live_count) only (see
 * ngp_nerf_composite_loss_live): input gradients are written for those rows,
 * the others are left as they were (and their inputs are not read). Only the
 * first ngp_reduce::live_slab_rows workgroups write a dW partial: a caller
 * that reduces with ngp_ffmlp_reduce, which takes no live count, zeroes the
 * workspaces first. */
int ngp_nerf_backward_live(const void* g_color_out, const void* color_in, const void* color_image, void* g_h,
                           const void* enc, const void* sigma_image, void* g_enc, uint32_t B,
                           const int32_t* live_rows, const int32_t* live_count, uint32_t hidden_dim,
                           uint32_t num_layers, uint32_t hidden_dim_color, uint32_t num_layers_color,
                           void* sigma_workspace, size_t sigma_workspace_bytes, void* color_workspace,
                           size_t color_workspace_bytes, uint32_t* timing, void* stream);
/* ngp_nerf_backward_live with a light regime for few live rows. With
 * 0 < *live_count <= min(dw_rows_max, whole 32-row chunks of dw_stash_rows,
 * 32 rows per workgroup of the launch: ceil(ceil(B / 32) / 4), at most 256)
 * the launch forms no dW: it writes g_h[:, 1:16] and g_enc exactly as
 * ngp_nerf_backward_live does (bit for bit) and stashes, per 32-row chunk and
 * transposed, the operands of the dW products (output gradients, inputs,
 * hidden post-activations and deltas; rows of the last chunk past the count
 * as zeros) in dw_stash (ngp_nerf_dw_stash_bytes(dw_stash_rows, ..) bytes,
 * scratch: nothing is read from it), and leaves the workspaces untouched. The
 * weight gradients are then formed from the stash, summed in fp32 in the slab
 * path's own order (one chunk per workgroup: the same bits as
 * ngp_nerf_backward_live + ngp_ffmlp_reduce), by
 * ngp_nerf_dw_reduce or by the bin launch of
 * ngp_grid_encode_backward_fused_dw_batch_live, called with the same stash,
 * rows and dw_rows_max. With more rows, or dw_rows_max 0, the launch is
 * ngp_nerf_backward_live's, dW partials included, and those two calls reduce
 * them as ngp_ffmlp_reduce does: every output bit-identical. The regime is
 * chosen on the device from *live_count. tests/test_gpu_nerf_dw.py. */
size_t ngp_nerf_dw_stash_bytes(uint32_t rows, uint32_t num_layers, uint32_t num_layers_color);
int ngp_nerf_backward_live_dw(const void* g_color_out, const void* color_in, const void* color_image, void* g_h,
                              const void* enc, const void* sigma_image, void* g_enc, uint32_t B,
                              const int32_t* live_rows, const int32_t* live_count, uint32_t hidden_dim,
                              uint32_t num_layers, uint32_t hidden_dim_color, uint32_t num_layers_color,
                              void* sigma_workspace, size_t sigma_workspace_bytes, void* color_workspace,
                              size_t color_workspace_bytes, uint32_t* timing, void* dw_stash,
                              uint32_t dw_stash_rows, uint32_t dw_rows_max, void* stream);
/* ngp_nerf_backward_live_dw with the list's join in the same launch: the
 * arguments are the per-ray lists ngp_nerf_composite_loss_lists leaves (rays
 * [N,3], live_cnt [N] 16-byte aligned, ray_rows [B]) instead of a finished
 * list. Every workgroup sums the counts, finds the list positions of its own
 * chunks and keeps their rows in LDS; it also stores them to live_rows, and
 * workgroup 0 stores live_total, so live_rows[0, *live_total), *live_total and
 * every output are those of ngp_nerf_composite_loss_live +
 * ngp_nerf_backward_live_dw bit for bit (entries of live_rows past the total
 * are not written). No workgroup waits for another. One pass holds
 * ngp_nerf_backward_join_max_rays() rays (4096) and B <= 262144 rows (32
 * chunks per workgroup): beyond either the call returns NGP_ERR_ARG and
 * launches nothing. tests/test_gpu_live_join.py. */
int ngp_nerf_backward_join_dw(const void* g_color_out, const void* color_in, const void* color_image, void* g_h,
                              const void* enc, const void* sigma_image, void* g_enc, uint32_t B,
                              const int32_t* rays, uint32_t N, const int32_t* live_cnt, const int32_t* ray_rows,
                              int32_t* live_rows, int32_t* live_total, uint32_t hidden_dim, uint32_t num_layers,
                              uint32_t hidden_dim_color, uint32_t num_layers_color, void* sigma_workspace,
                              size_t sigma_workspace_bytes, void* color_workspace, size_t color_workspace_bytes,
                              uint32_t* timing, void* dw_stash, uint32_t dw_stash_rows, uint32_t dw_rows_max,
                              void* stream);
uint32_t ngp_nerf_backward_join_max_rays(void);
/* The weight gradients (fp16) of ngp_nerf_backward_live_dw in one launch:
 * network 0 the sigma network, 1 the colour network (workspaces, Bs = the
 * backward's B twice, shapes and grad_weights as ngp_ffmlp_reduce lists them).
 * Light regime: the products from the stash (exact zeros with
 * *live_count <= 0); otherwise the slab reduce over the live rows' slab rows.
 * nonfinite (nullable): set to 1 when a written grad is inf/nan. */
int ngp_nerf_dw_reduce(void* const* workspaces, const uint32_t* Bs, const uint32_t* in_dims,
                       const uint32_t* hidden_dims, const uint32_t* num_layers, void* const* grad_weights,
                       int32_t* nonfinite, const int32_t* live_count, const void* dw_stash,
                       uint32_t dw_stash_rows, uint32_t dw_rows_max, void* stream);
/* ngp_grid_encode_backward_fused_reduce_batch_live (src null) or
 * .._reduce_batch_images (src given, live_rows required here) after
 * ngp_nerf_backward_live_dw: in the light regime the first workgroups of the
 * bin launch's slab-reduce column, one per 16x16 tile of the two networks'
 * dW, form the weight gradients from the stash (ngp_nerf_dw_reduce's values
 * bit for bit) and the column's other workgroups return at once; in the other
 * regime the column is the slab reduce, the launch that of
 * .._reduce_batch_live. n_nets 2: sigma, colour. */
int ngp_grid_encode_backward_fused_dw_batch_live(
    const void* grad, const float* xyz, float bound, const int32_t* offsets, void* grad_embeddings, uint32_t B,
    const int32_t* live_rows, const int32_t* live_count, uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H,
    uint32_t gridtype, int32_t align_corners, uint32_t interp, const int32_t* offsets_host, void* workspace,
    size_t workspace_bytes, int32_t grad_layout, int32_t* nonfinite, int32_t n_nets, void* const* mlp_workspaces,
    const uint32_t* mlp_Bs, const uint32_t* in_dims, const uint32_t* hidden_dims, const uint32_t* num_layers,
    void* const* grad_weights, int32_t* mlp_nonfinite, const ngp_batch_job* job, const ngp_image_source* src,
    const void* dw_stash, uint32_t dw_stash_rows, uint32_t dw_rows_max, void* stream);
/* Sums the deferred dW partials of n backward calls (same B and shapes as
 * those calls) into grad_weights[k], in one launch (n <= 4). nonfinite
 * (nullable): set to 1 when a written grad is inf/nan (GradScaler's check). */
int ngp_ffmlp_reduce(int32_t n, void* const* workspaces, const uint32_t* Bs, const uint32_t* in_dims,
                     const uint32_t* hidden_dims, const uint32_t* num_layers,
                     void* const* grad_weights, int32_t gw_dtype, int32_t* nonfinite, void* stream);
size_t ngp_fused_state_bytes(void);
int ngp_fused_state_init(void* state, float init_scale, void* stream);
/* Synthetic Lego batch (nerf/provider.py SyntheticLego): boxes = nboxes x
 * (lo[3], hi[3], rgb[3]); poses [n_poses, 4, 4]; intrinsics (fx, fy, cx, cy).
 * The batch index is the state's own draw counter. Also records the previous
 * batch's counter[0..1] into step_counter[(draw - 1) % 16] (nullable; the
 * reference's per-step record for update_extra_state) and zeroes counter for
 * the marcher. Touches no state the optimizer uses, so it may run beside
 * ngp_fused_optimizer_step of the previous step. */
int ngp_lego_rays(const float* poses, uint32_t n_poses, const float* intrinsics4, uint32_t H,
                  uint32_t W, uint32_t N, const float* boxes, int32_t nboxes, const float* aabb6,
                  float min_near, uint32_t seed, void* state, float* rays_o, float* rays_d,
                  float* rgba, float* bg, float* nears, float* fars, float* noises,
                  int32_t* counter, int32_t* step_counter, void* stream);
int ngp_nerf_glue_forward(const void* h_sigma, const float* dirs, float density_scale, float* sigma,
                          void* color_in, uint32_t B, const int32_t* count, void* stream);
int ngp_nerf_glue_backward(const void* grad_color_in, void* grad_h_sigma, uint32_t B,
                           const int32_t* count, void* stream);
int ngp_nerf_composite_loss(const float* sigma, const void* color_out, const void* h_sigma,
                            const float* deltas, const int32_t* rays, uint32_t M, uint32_t N,
                            float T_thresh, float density_scale, const float* gt,
                            uint32_t gt_channels, const float* bg, void* state,
                            void* grad_color_out, void* grad_h_sigma, float* out_image,
                            float* out_ws, float* loss_ray, void* stream);
/* ngp_nerf_composite_loss plus the step's live rows: every row whose written
 * gradient (the colour logits' and the density's) is nonzero in some
 * component, listed in ray order in live_rows [M] (live_total[0] of them);
 * ray_rows [M] and live_cnt [N] are scratch (each ray's live rows in its own
 * row range, and their count). The other rows' gradients are exactly zero, so
 * the backwards may skip them (ngp_nerf_backward_live,
 * ngp_grid_encode_backward_fused_reduce_batch_live): the products with a zero
 * row are zeros (instant-ngp compacts its samples before the backward the same
 * way). Two launches. */
int ngp_nerf_composite_loss_live(const float* sigma, const void* color_out, const void* h_sigma,
                                 const float* deltas, const int32_t* rays, uint32_t M, uint32_t N, float T_thresh,
                                 float density_scale, const float* gt, uint32_t gt_channels, const float* bg,
                                 void* state, void* grad_color_out, void* grad_h_sigma, float* out_image,
                                 float* out_ws, float* loss_ray, int32_t* ray_rows, int32_t* live_cnt,
                                 int32_t* live_rows, int32_t* live_total, void* stream);
/* ngp_nerf_composite_loss_live's first launch alone: the per-ray lists
 * ray_rows [M] (ray n's live rows, in order, from its first row rays[3 n + 1])
 * and live_cnt [N] (their count; 0 for a ray dropped for overflowing M; 16-byte
 * aligned), for a backward that joins the list itself
 * (ngp_nerf_backward_join_dw). One launch. */
int ngp_nerf_composite_loss_lists(const float* sigma, const void* color_out, const void* h_sigma,
                                  const float* deltas, const int32_t* rays, uint32_t M, uint32_t N, float T_thresh,
                                  float density_scale, const float* gt, uint32_t gt_channels, const float* bg,
                                  void* state, void* grad_color_out, void* grad_h_sigma, float* out_image,
                                  float* out_ws, float* loss_ray, int32_t* ray_rows, int32_t* live_cnt,
                                  void* stream);
/* The depth-supervised loss (the reference's train_step, nerf/utils.py:545-553
 * and :951-954): per ray, with pred the composite's own depth (0 for a ray
 * without samples or dropped for overflowing M),
 *   mask = depth_min <= gt && gt <= depth_max     (model.min_near, model.bound)
 *   dep  = mask ? |gt - max(pred, 0)| : 0
 *   loss_ray[n] = color_weight * mse + depth_weight * dep
 * The colour gradients are scaled by color_weight, and the depth gradient
 * scale * depth_weight / N * sign(pred - gt) (0 outside the mask, sign(0) = 0)
 * reaches the densities through the composite backward (raymarching.cu:674).
 * dep is a select where the reference multiplies by the mask: a masked ray
 * (a NaN or inf target too) contributes exactly +0 here.
 *   gt_depth f32 [N] by ray index, ngp units (nullable with depth_weight 0:
 *     every ray masked); out_depth (nullable) f32 [N] by ray index: pred;
 *   loss_depth_ray (nullable) f32 [N], ray n's unweighted dep;
 *   ray_rows / live_cnt / live_rows / live_total: all four as
 *     ngp_nerf_composite_loss_live lists the live rows, or all four null. */
typedef struct ngp_depth_loss_job {
    const float* gt_depth;
    float color_weight, depth_weight;
    float depth_min, depth_max;
    float* out_depth;
    float* loss_depth_ray;
    int32_t *ray_rows, *live_cnt, *live_rows, *live_total;
} ngp_depth_loss_job;
/* ngp_nerf_composite_loss (live lists null) / ngp_nerf_composite_loss_live with
 * the job's loss. color_weight 1 and depth_weight 0 give those entries' outputs
 * bit for bit. */
int ngp_nerf_composite_loss_depth(const float* sigma, const void* color_out, const void* h_sigma,
                                  const float* deltas, const int32_t* rays, uint32_t M, uint32_t N, float T_thresh,
                                  float density_scale, const float* gt, uint32_t gt_channels, const float* bg,
                                  void* state, void* grad_color_out, void* grad_h_sigma, float* out_image,
                                  float* out_ws, float* loss_ray, const ngp_depth_loss_job* job, void* stream);
/* .._depth as ngp_nerf_composite_loss_lists: the job's ray_rows and live_cnt are
 * required and written, its live_rows and live_total are not used. One launch. */
int ngp_nerf_composite_loss_depth_lists(const float* sigma, const void* color_out, const void* h_sigma,
                                        const float* deltas, const int32_t* rays, uint32_t M, uint32_t N,
                                        float T_thresh, float density_scale, const float* gt, uint32_t gt_channels,
                                        const float* bg, void* state, void* grad_color_out, void* grad_h_sigma,
                                        float* out_image, float* out_ws, float* loss_ray,
                                        const ngp_depth_loss_job* job, void* stream);
/* The distortion regulariser of mip-NeRF 360 in its O(n) form (the reference's
 * loss.py EffDistLoss), on the composite's own weights: per ray, with
 * delta_i = deltas[i][0], m_i the composite's t (the running sum of
 * deltas[.][1]) and w_i the composite's weight (0 past the early stop),
 *   dist = sum_ij w_i w_j |m_i - m_j| + 1/3 sum_i delta_i w_i^2
 * in ngp units; 0 for a ray without samples or dropped for overflowing M.
 *   loss_ray[n] = the depth entry's value + weight * dist
 * and scale * weight / N * d dist / d sigma is added to the density gradient
 * before its one rounding to half. weight 0: dist is still computed and
 * written, the loss, the gradients and the live lists are the depth entry's
 * bit for bit. */
typedef struct ngp_dist_loss_job {
    float weight;          /* >= 0 */
    float* loss_dist_ray;  /* nullable f32 [N], ray n's unweighted dist (by list position, as loss_ray) */
} ngp_dist_loss_job;
/* ngp_nerf_composite_loss_depth plus the distortion term. job is required and
 * keeps its meaning (color_weight 1, depth_weight 0 and a null gt_depth give
 * the colour-only loss; it carries the live lists). A null dist, or a negative
 * or non-finite weight: NGP_ERR_ARG before any device work. */
int ngp_nerf_composite_loss_dist(const float* sigma, const void* color_out, const void* h_sigma,
                                 const float* deltas, const int32_t* rays, uint32_t M, uint32_t N, float T_thresh,
                                 float density_scale, const float* gt, uint32_t gt_channels, const float* bg,
                                 void* state, void* grad_color_out, void* grad_h_sigma, float* out_image,
                                 float* out_ws, float* loss_ray, const ngp_depth_loss_job* job,
                                 const ngp_dist_loss_job* dist, void* stream);
/* .._dist as ngp_nerf_composite_loss_depth_lists. One launch. */
int ngp_nerf_composite_loss_dist_lists(const float* sigma, const void* color_out, const void* h_sigma,
                                       const float* deltas, const int32_t* rays, uint32_t M, uint32_t N,
                                       float T_thresh, float density_scale, const float* gt, uint32_t gt_channels,
                                       const float* bg, void* state, void* grad_color_out, void* grad_h_sigma,
                                       float* out_image, float* out_ws, float* loss_ray,
                                       const ngp_depth_loss_job* job, const ngp_dist_loss_job* dist, void* stream);
/* scaler_enabled of the optimizer entries: GradScaler off; on, with its inf
 * check as a sweep over the grads; on, with the check already made by the
 * kernels that wrote the grads into the state's flag (ngp_fused_inf_flag). */
#define NGP_SCALER_OFF 0
#define NGP_ADAM_SHADOW_ALL 2
#define NGP_SCALER_SCAN 1
#define NGP_SCALER_PRECHECKED 2
/* The state's GradScaler flag (local == 0: the found-inf flag the optimizer
 * reads; local != 0: the data-parallel guard's per-rank flag), for the
 * nonfinite arguments of the grid backward and the MLP reduce. */
int32_t* ngp_fused_inf_flag(void* state, int32_t local);
/* Adam (+ GradScaler inf check/unscale/update, LambdaLR 0.1^(epoch/iters))
 * over n_tensors fp32 params with fp16 grads; half_params[k] (nullable) is
 * refreshed with half(p) where the update changed p (every value with
 * zero_grads | NGP_ADAM_SHADOW_ALL: a shadow written only now and then);
 * grads are zeroed when zero_grads & 1;
 * grads are multiplied by grad_mult as well as unscaled (data-parallel mean).
 * step_counter (nullable; pass null when ngp_lego_rays records it) gets
 * counter[0..1] at slot iter % 16. */
int ngp_fused_optimizer_step(int32_t n_tensors, float* const* params, void* const* grads,
                             float* const* exp_avg, float* const* exp_avg_sq,
                             void* const* half_params, const uint64_t* sizes, float lr, float beta1,
                             float beta2, float eps, int32_t iters, int32_t zero_grads,
                             float grad_mult, float growth_factor, float backoff_factor,
                             int32_t growth_interval,
                             int32_t scaler_enabled, uint32_t num_rays, const int32_t* counter,
                             int32_t* step_counter, const float* loss_ray, void* state,
                             void* stream);
/* ngp_fused_optimizer_step without its bookkeeping launch: the GradScaler
 * update, LR epoch, step counts and loss of this update are marked pending in
 * `state` and done by the next ngp_fused_step_head (the fused step's first
 * launch), saving one latency-bound single-block launch per step. */
int ngp_fused_optimizer_update(int32_t n_tensors, float* const* params, void* const* grads,
                               float* const* exp_avg, float* const* exp_avg_sq, void* const* half_params,
                               const uint64_t* sizes, float lr, float beta1, float beta2, float eps,
                               int32_t iters, int32_t zero_grads, float grad_mult, int32_t scaler_enabled,
                               void* state, void* stream);
/* The fused step's first launch: ngp_lego_rays's batch (same arguments), the
 * pending bookkeeping of the last ngp_fused_optimizer_update if any (scaler
 * arguments as ngp_fused_optimizer_step; loss_ray holds the previous batch's
 * per-ray losses, N rays), and ngp_ffmlp_pack of n_nets networks (n_nets may
 * be 0), as disjoint block ranges of one kernel; it also zeroes clear_bytes
 * (a multiple of 16) at clear (nullable: the grid backward's bin cursors). */
int ngp_fused_step_head(const float* poses, uint32_t n_poses, const float* intrinsics4, uint32_t H,
                        uint32_t W, uint32_t N, const float* boxes, int32_t nboxes, const float* aabb6,
                        float min_near, uint32_t seed, void* state, float* rays_o, float* rays_d,
                        float* rgba, float* bg, float* nears, float* fars, float* noises, int32_t* counter,
                        int32_t* step_counter, float growth_factor, float backoff_factor,
                        int32_t growth_interval, int32_t scaler_enabled, const float* loss_ray,
                        int32_t n_nets, const void* const* mlp_weights, const uint32_t* in_dims,
                        const uint32_t* hidden_dims, const uint32_t* num_layers, void* const* images,
                        void* clear, uint32_t clear_bytes, void* stream);
/* ngp_fused_optimizer_update (bookkeeping deferred) and the batch + clear
 * parts of ngp_fused_step_head (same arguments) as block ranges of one launch;
 * the deferred bookkeeping and the MLP packs then go to
 * ngp_march_rays_train_prebuilt_tail. */
int ngp_fused_optimizer_update_head(int32_t n_tensors, float* const* params, void* const* grads,
                                    float* const* exp_avg, float* const* exp_avg_sq,
                                    void* const* half_params, const uint64_t* sizes, float lr, float beta1,
                                    float beta2, float eps, int32_t iters, int32_t zero_grads,
                                    float grad_mult, int32_t scaler_enabled, void* state,
                                    const float* poses, uint32_t n_poses, const float* intrinsics4,
                                    uint32_t H, uint32_t W, uint32_t N, const float* boxes, int32_t nboxes,
                                    const float* aabb6, float min_near, uint32_t seed, float* rays_o,
                                    float* rays_d, float* rgba, float* bg, float* nears, float* fars,
                                    float* noises, int32_t* counter, int32_t* step_counter, void* clear,
                                    uint32_t clear_bytes, void* stream);

/* Data-parallel GradScaler guard for the sharded optimizer (nerf/fused.py,
 * world > 1), run on each rank's own fp16 gradient before the averaging
 * reduce-scatter: if any of its n elements is inf/nan, a NaN is written to
 * grad[r * chunk] for r in [0, world), so every rank's shard of the reduced
 * gradient carries it and every rank's ngp_fused_optimizer_step skips.
 * n % 8 == 0, grad 16-byte aligned, world * chunk <= n. No reference
 * counterpart (the reference trains on one GPU; GradScaler.unscale_ checks
 * the whole gradient, torch/amp/grad_scaler.py). */
int ngp_grad_guard(void* grad_half, uint64_t n, uint64_t chunk, int32_t world, void* state,
                   void* stream);
/* (n == 0: no scan; the per-rank flag ngp_fused_inf_flag(state, 1) was set by
 * the kernels that wrote the gradient.) */

/* Touched-entry gradient exchange of the replicated data-parallel step
 * (nerf/exchange.py; DESIGN.md §7 option B). Replaces the reference's DDP
 * gradient all-reduce (nerf/utils.py:325-327) for the fused engine: each rank
 * lists its nonzero fp16 channel pairs, the lists (fixed size, so the step
 * captures whole) are all-gathered, and every rank sums all of them exactly
 * (int64, 2^-24 fixed point) into the same flat gradient, then runs the full
 * Adam (world 1's step).
 *   list: grad_half[n_values] (16-byte aligned, n_values % 8 == 0) -> send,
 *     ngp_grad_exchange_words(n_values, cap) int64 words: header (int32
 *     count, int32 flags: bit 0 a non-finite value or *inf_flag (nullable)
 *     set; the header must be zero before the call), a table of
 *     bins(n_values) words ((count << 32) | start) and up to cap items
 *     ((half2 bits << 32) | pair index). The gradient is not changed.
 *   reduce: recv = world lists back to back -> grad_half = fp16(sum / world)
 *     over every value (dense); any rank's flag -> *inf_flag |= 1; a list over
 *     cap -> *inf_flag |= 2 (the update is skipped without a scale back-off)
 *     and grad_half zeroed; stats[0] += 1 per overflowed exchange, stats[1] =
 *     max(stats[1], the largest count); send (nullable): this rank's list,
 *     whose header is cleared for the next list call. */
uint32_t ngp_grad_exchange_bins(uint64_t n_values);
uint64_t ngp_grad_exchange_words(uint64_t n_values, uint32_t cap);
int ngp_grad_exchange_list(const void* grad_half, uint64_t n_values, const int32_t* inf_flag, void* send,
                           uint32_t cap, void* stream);
int ngp_grad_exchange_reduce(const void* recv, int32_t world, uint32_t cap, void* grad_half, uint64_t n_values,
                             int32_t* inf_flag, int32_t* stats, void* send, void* stream);

/* ------------------------------------------------------------------------ */
/* Density-grid update (replaces the torch glue of NeRFRenderer.             */
/* update_extra_state, nerf/renderer.py:498-598, and its packbits call,      */
/* raymarching.h:11)                                                          */
/* ------------------------------------------------------------------------ */

/* Every entry below that takes a grid shape requires 1 <= C <= 16 cascades and
 * H a power of two in [2, 1024] with C * H^3 < 2^32 (a cell's index is
 * cascade * H^3 + its Morton code, below H^3 only for a power of two), and
 * returns NGP_ERR_ARG otherwise. The threshold is Python's min(mean_density,
 * density_thresh): a NaN mean stays NaN and clears every bit. */

/* The query points of one update, P = C * ppc ordered by cascade. coords
 * int32 [P,3] cell coordinates (renderer.py:552-561), or NULL for every cell
 * of each cascade in meshgrid(x, y, z, 'ij') order (ppc = H^3, :516-523);
 * noise f32 [P,3] uniform [0,1) (the reference's rand_like, :533 / :569).
 * Writes xyzs f32 [P,3] = (2c/(H-1) - 1)(bound_c - hgs) + (2 noise - 1) hgs
 * with the reference's fp32 operations, and indices i32 [P] = cascade * H^3 +
 * morton3D(c). */
int ngp_density_grid_points(const int32_t* coords, const float* noise, uint32_t P, uint32_t ppc, uint32_t C,
                            uint32_t H, float bound, float* xyzs, int32_t* indices, void* stream);
/* The points [lo, hi) of the same draws (coords required), written to xyzs /
 * indices [0, hi - lo) in brick order: bucketed by cascade and morton3D(c) >>
 * shift (bricks of >= 512 cells, at most 8192 buckets), in unspecified order
 * inside a bucket. The densities' max into tmp_grid does not depend on the
 * order, so an update gives the same grid as with ngp_density_grid_points,
 * while a wave's points share the coarse levels' cache lines in the query.
 * ws: ngp_density_grid_sort_workspace_bytes(C, H) bytes (cleared here). */
size_t ngp_density_grid_sort_workspace_bytes(uint32_t C, uint32_t H);
int ngp_density_grid_points_sorted(const int32_t* coords, const float* noise, uint32_t P, uint32_t ppc, uint32_t C,
                                   uint32_t H, float bound, uint32_t lo, uint32_t hi, void* ws, size_t ws_bytes,
                                   float* xyzs, int32_t* indices, void* stream);
/* The densities of the points: sigma network forward on their encodings
 * (pair-major [L][B][2] half, ngp_grid_encode_forward_fused out_layout 0),
 * density = exp(h[:,0]) * density_scale (renderer.py:535-536), written as a
 * max into tmp_grid[indices[b]] (tmp_grid f32 [C * H^3], -1 where unset;
 * a cell drawn twice keeps the larger density). image: ngp_ffmlp_pack image
 * of the network or NULL. With an image and in_dim 32 the streaming kernel
 * runs (hidden 32 / 64, num_layers 2..4); every other shape of the FFMLP, and
 * a NULL image, takes the generic kernel. tests/test_gpu_nerf_net.py (case f)
 * holds both, and ngp_nerf_density_forward_rows, to the float64 oracle on all
 * of these shapes; the trainer's 64 / 2 also in tests/test_gpu_density.py. */
int ngp_nerf_density_forward(const void* inputs, const void* weights, const void* image, uint32_t B,
                             uint32_t in_dim, uint32_t hidden_dim, uint32_t num_layers, float density_scale,
                             const int32_t* indices, float* tmp_grid, void* stream);
/* The same densities stored per row, sigma[b] (no index, no atomic): the full
 * update's Morton-ordered queries (row = cell) and the brick-ordered partial
 * queries (then ngp_density_grid_run_max). 32 inputs, image required. */
int ngp_nerf_density_forward_rows(const void* inputs, const void* image, uint32_t B, uint32_t hidden_dim,
                                  uint32_t num_layers, float density_scale, float* sigma, void* stream);
/* EMA (renderer.py:582-583: where grid >= 0 and tmp >= 0, grid = max(grid *
 * decay, tmp)), tmp reset to -1, stats[0] = sum(clamp(grid, 0)) as a double
 * (mean_density = float(stats[0] / (C H^3)), :584), and the bitfield at
 * min(mean_density, density_thresh) (:589-590), all on the device. stats:
 * NGP_DENSITY_STATS_LEN doubles (the sum, then per-block partial sums added
 * in a fixed order: no atomics, no clear). */
#define NGP_DENSITY_STATS_LEN 1025
int ngp_density_grid_ema_pack(float* grid, float* tmp_grid, uint32_t C, uint32_t H, float decay,
                              double density_thresh, double* stats, uint8_t* bitfield, void* stream);
/* Device-side draws of an update (no host sync, graph-capturable): partial=0:
 * the noise of every cell (coords unused); partial=1: per cascade H^3/4
 * uniform cells then H^3/4 cells drawn from the cascade's occupied cells
 * (grid > 0, listed in cell order as torch.nonzero does, :555-558), with
 * their noise. Counter RNG over (seed ^ 0xd3a5b1c7, update, point): its own
 * domain, apart from the training sampler's draws of the same seed. */
size_t ngp_density_grid_draw_workspace_bytes(uint32_t C, uint32_t H);
int ngp_density_grid_draw(const float* grid, uint32_t C, uint32_t H, uint32_t partial, uint32_t seed,
                          uint32_t update, int32_t* coords, float* noise, void* ws, size_t ws_bytes,
                          void* stream);
/* A partial update's draws for the fused trainer, generated in Morton order:
 * per cascade N = H^3/4 uniform cells and N cells out of the occupied list
 * (grid > 0), i.i.d. with replacement as the reference draws them
 * (renderer.py:548-558), made as uniform order statistics (prefix sums of N+1
 * exponentials from the counter RNG, exact 2^-32 fixed point), so each half's
 * cells come out sorted by Morton code with no sort; the points [lo, hi) of
 * the C * 2N draws (cascade-major, uniform half first) are written to xyzs /
 * indices [0, hi - lo) with k_density_points' arithmetic. H a power of two.
 * draw_ws: ngp_density_grid_draw_workspace_bytes; ostat_ws:
 * ngp_density_grid_ostat_workspace_bytes. */
size_t ngp_density_grid_ostat_workspace_bytes(uint32_t C, uint32_t H);
int ngp_density_grid_draw_sorted(const float* grid, uint32_t C, uint32_t H, uint32_t seed, uint32_t update,
                                 float bound, uint32_t lo, uint32_t hi, void* draw_ws, size_t draw_ws_bytes,
                                 void* ostat_ws, size_t ostat_ws_bytes, float* xyzs, int32_t* indices, void* stream);
/* tmp_grid from the densities sigma[0, hi - lo) of ngp_density_grid_draw_sorted's
 * points [lo, hi): a cell's draws are adjacent within a half, so each run's
 * max is folded in by its first point with one integer atomic max (exact, in
 * any order). tmp_grid holds -1 where nothing was drawn (as the EMA leaves
 * it); densities are >= 0. */
int ngp_density_grid_run_max(const float* sigma, const int32_t* indices, uint32_t C, uint32_t H, uint32_t lo,
                             uint32_t hi, float* tmp_grid, void* stream);
/* mean_count after an update (renderer.py:593-595: int(mean of the last
 * min(16, local_step) batches' sample counts)) on the device: *out = floor(sum
 * / total) over the fused trainer's step-counter ring (int32 [16][2], slot =
 * batch % 16; *draw = batches drawn; ahead: the newest batch is in the ring,
 * else in counter[0]). */
int ngp_density_mean_count(const int32_t* step_counter, const int32_t* draw, const int32_t* counter,
                           uint32_t total, uint32_t ahead, int64_t* out, void* stream);

/* ------------------------------------------------------------------------ */
/* Mesh export (replaces extract_fields / extract_geometry, nerf/utils.py    */
/* :172-202, and the PyMCubes call of Trainer.save_mesh, :688-708)           */
/* ------------------------------------------------------------------------ */

/* Conventions of the three entries: a lattice of nx x ny x nz points, index
 * p = (i * ny + j) * nz + k (meshgrid(x, y, z, 'ij') order, utils.py:183-186);
 * a cell is named by its minimum corner; a point is inside when value >=
 * threshold (NaN: outside, read as 0 by the interpolation). aabb: six floats
 * on the host, min then max. Errors are found before any device work:
 * NGP_ERR_ARG for a resolution below 2, nx * ny * nz >= 2^31, a null
 * required pointer, a workspace that is too small, a non-finite threshold or
 * an aabb with max <= min; NGP_ERR_UNSUPPORTED for V or T >= 2^31. */

/* The world positions of lattice points [lo, hi), xyzs f32 [hi - lo, 3]: per
 * axis min + (max - min) * ((float)i / (float)(n - 1)) in fp32, the points
 * extract_fields draws with torch.linspace for extract_geometry and
 * Trainer.save_mesh (nerf/utils.py:172-202, :688-708). */
int ngp_mesh_lattice_points(uint32_t nx, uint32_t ny, uint32_t nz, const float* aabb, uint32_t lo, uint32_t hi,
                            float* xyzs, void* stream);
/* Marching cubes over volume f32 [nx, ny, nz] (the mcubes.marching_cubes call
 * of extract_geometry, nerf/utils.py:172-202, for save_mesh, :688-708), pass 1: per lattice point the crossed +x / +y /
 * +z edges and its cell's triangle count, then their exclusive scans into
 * the workspace (no atomics: the order below is fixed and two runs give the
 * same bytes). counts: device uint64[2], the vertex and triangle totals V, T;
 * the caller reads them to allocate the outputs of ngp_mesh_emit. */
size_t ngp_mesh_workspace_bytes(uint32_t nx, uint32_t ny, uint32_t nz);
int ngp_mesh_count(const float* volume, uint32_t nx, uint32_t ny, uint32_t nz, float threshold, void* ws,
                   size_t ws_bytes, uint64_t* counts, void* stream);
/* Pass 2, on the workspace ngp_mesh_count filled from the same volume and
 * threshold: vertices f32 [V, 3] ordered by (p, axis), each on the edge from p
 * along axis at t = (threshold - a) / (b - a), a the value at p and b at the
 * +axis neighbour, in lattice units as mcubes returns them (aabb NULL) or
 * mapped per axis by min + (max - min) * (pos / (n - 1)) (nerf/utils.py:172-202,
 * the mapping at :198-201; the vertices and triangles save_mesh, :688-708, exports);
 * faces int32 [T, 3] ordered by (cell, case-table order), normals pointing
 * from inside to outside; normals f32 [V, 3] or NULL: the normalised negative
 * gradient of the volume (central differences, one-sided on the border). V =
 * T = 0: nothing is launched. */
int ngp_mesh_emit(const float* volume, uint32_t nx, uint32_t ny, uint32_t nz, float threshold, const float* aabb,
                  const void* ws, size_t ws_bytes, uint64_t V, uint64_t T, float* vertices, float* normals,
                  int32_t* faces, void* stream);

/* After the extraction: connected components, cleaning and vertex colours of
 * an indexed triangle mesh (vertices f32 [V, 3], faces int32 [T, 3], normals
 * f32 [V, 3]). No reference counterpart: its save_mesh, :688-708, hands the
 * arrays to trimesh unprocessed. Common to the entries: V or T >= 2^31 is
 * NGP_ERR_UNSUPPORTED, a null required pointer NGP_ERR_ARG, both before any
 * device work; a triangle with an index outside [0, V) is never dereferenced,
 * belongs to no component and is dropped by the clean. Integer atomics only,
 * with order-independent results, and no kernel waits for another thread. */

/* labels int32 [V]: the smallest vertex index of v's component (two vertices
 * are connected when a triangle holds both; a vertex no triangle uses is a
 * component of its own). comp_faces int32 [V]: at a label the number of
 * triangles of its component, 0 elsewhere. Lock-free union-find in labels,
 * three launches (init, hook, compress + count); DESIGN.md §20 has the
 * invariant. V = 0: nothing is launched; T = 0: faces is not read. */
int ngp_mesh_components(const int32_t* faces, uint64_t V, uint64_t T, int32_t* labels, int32_t* comp_faces,
                        void* stream);
/* Cleaning, pass 1, on ngp_mesh_components' labels and comp_faces. A component
 * is kept when comp_faces >= min_faces and, with keep_largest, it is also the
 * one with the most triangles (a tie: the smaller label). A triangle is kept
 * when its indices are valid and its component is kept; a vertex when a kept
 * triangle uses it (so unreferenced vertices go too). The kept flags and their
 * exclusive scans go to the workspace (placement by scans, no atomics: the
 * original order is kept and two runs give the same bytes). counts: device
 * uint64[4] = V', T', the components before, the components the rule keeps;
 * the caller reads them once to allocate the outputs of ngp_mesh_clean_emit.
 * 0 from ngp_mesh_clean_workspace_bytes: V or T >= 2^31. */
size_t ngp_mesh_clean_workspace_bytes(uint64_t V, uint64_t T);
int ngp_mesh_clean_count(const int32_t* faces, uint64_t V, uint64_t T, const int32_t* labels,
                         const int32_t* comp_faces, uint32_t min_faces, int32_t keep_largest, void* ws,
                         size_t ws_bytes, uint64_t* counts, void* stream);
/* Pass 2, on the workspace ngp_mesh_clean_count filled from the same mesh:
 * vertices_out f32 [V2, 3] and normals_out f32 [V2, 3] (nullable, needs
 * normals) are the kept vertices in their original order, faces_out int32
 * [T2, 3] the kept triangles in theirs with the indices remapped. V2 = T2 = 0:
 * nothing is launched. V2 > V or T2 > T: NGP_ERR_ARG. */
int ngp_mesh_clean_emit(const float* vertices, const float* normals, const int32_t* faces, uint64_t V, uint64_t T,
                        const void* ws, size_t ws_bytes, uint64_t V2, uint64_t T2, float* vertices_out,
                        float* normals_out, int32_t* faces_out, void* stream);
/* The view directions of a vertex colour query, dirs f32 [n, 3] = -normal /
 * |normal| in fp32: a camera that looks straight at the surface. A normal
 * whose length is zero or not finite gives (0, 0, 1). */
int ngp_mesh_color_dirs(const float* normals, uint64_t n, float* dirs, void* stream);
/* rgb u8 [n, 3] from the first three of each row of `stride` halves: logits
 * != 0 (ngp_nerf_forward's color_out, stride 16): sigmoid 1 / (1 + expf(-x))
 * in fp32 first; then ngp_frame_finish's q(x) = (uint8)(clamp(x, 0, 1) *
 * 255.0f), truncating, 0 for a NaN. Exactly n rows are written. */
int ngp_mesh_color_finish(const void* values, uint32_t stride, uint64_t n, int32_t logits, uint8_t* rgb,
                          void* stream);

/* ------------------------------------------------------------------------ */
/* Whole frames around the device-driven render loop (replaces the per-frame */
/* get_rays + near_far + render_init before it and the blend / quantisation  */
/* of Trainer.test after it, nerf/utils.py:656-685, 743-796)                 */
/* ------------------------------------------------------------------------ */

/* One launch before the loop: all N = H * W rays of pose `pose_index` of the
 * device stack poses f32 [n_poses, 4, 4], pixel p = row * W + col (get_rays
 * with N = -1, utils.py:52-136, in the arithmetic of the training draw,
 * ngp_image_rays, bit for bit), nears / fars as ngp_near_far_from_aabb gives
 * them, noises = 0, and what ngp_render_init sets: alive list 0 = arange(N),
 * rays_t = nears, weights_sum / depth / image = 0, the loop state.
 * intrinsics4 (fx, fy, cx, cy) and aabb6 are on the host. Buffers are [N] or
 * [N, 3], 16-byte aligned. Null buffers, H * W outside [1, 2^28), pose_index
 * >= n_poses or a misaligned buffer: NGP_ERR_ARG before any device work. */
int ngp_frame_begin(const float* poses, uint32_t n_poses, uint32_t pose_index, const float* intrinsics4, uint32_t H,
                    uint32_t W, const float* aabb6, float min_near, float* rays_o, float* rays_d, float* nears,
                    float* fars, float* noises, int32_t* rays_alive, float* rays_t, float* weights_sum, float* depth,
                    float* image, void* state, void* stream);
/* One launch after the loop has ended, per pixel p:
 *   c = image[p] + (1 - weights_sum[p]) * bg_color       (each of 3 channels)
 *   z = max(depth[p] - nears[p], 0) / (fars[p] - nears[p])  (a NaN stays one;
 *       a ray that misses the box has near == far: 0 / 0)
 * in fp32 without contraction, then rgb8 u8 [H, W, 3] = q(c), depth8 u8 [H, W]
 * = q(z) with q(x) = (uint8)(clamp(x, 0, 1) * 255.0f), truncating, 0 for a
 * non-finite x: the reference's (x * 255).astype(np.uint8), made total.
 * image_out f32 [N, 3] / depth_out f32 [N] (each nullable) receive c and z.
 * Float buffers 16-byte aligned, uint8 outputs 4-byte aligned. Null required
 * buffers, H * W outside [1, 2^28), misalignment: NGP_ERR_ARG. */
int ngp_frame_finish(uint32_t H, uint32_t W, const float* image, const float* weights_sum, const float* depth,
                     const float* nears, const float* fars, float bg_color, uint8_t* rgb8, uint8_t* depth8,
                     float* image_out, float* depth_out, void* stream);

/* The validation pass: one launch after the loop has ended, in place of
 * ngp_frame_finish. Per pixel p and channel j,
 *   c  = image[p][j] + (1 - weights_sum[p]) * bg_color      (ngp_frame_finish's c)
 *   gt = pixel p of image `pose_index` of src->pixels [n, H, W, channels],
 *        decoded as the training draw decodes it (uint8: v / 255, a true
 *        division; float32 as stored), RGBA blended on white in fp32:
 *        rgb * a + (1 - a)                                   (nerf.eval.ground_truth)
 *   d  = c - gt, d * d in fp32 without contraction,
 * and sse_out[pose_index] (double) = the sum of all 3 H W squares, added in
 * double: each thread adds the squares of its 4-pixel runs in pixel order, a
 * workgroup adds its threads in a fixed tree and stores one partial, and the
 * workgroup that finishes last (an integer ticket) adds the partials in index
 * order. No floating-point atomics: the sum depends on H * W alone and is
 * the same from run to run. A non-finite c makes the sum non-finite. Only
 * pixels, channels and dtype of src are read (its checks are the draw's);
 * the caller guarantees pose_index < n. The partials and the ticket are the
 * library's: one call at a time per device (calls on one stream are); the
 * entry clears the ticket on the stream before the launch, so a call does
 * not depend on how an earlier one ended. image
 * and weights_sum 16-byte aligned, sse_out 8-byte aligned. Null buffers, a
 * bad source, H * W outside [1, 2^28), misalignment: NGP_ERR_ARG. */
int ngp_frame_sse(uint32_t H, uint32_t W, const float* image, const float* weights_sum, float bg_color,
                  const ngp_image_source* src, uint32_t pose_index, double* sse_out, void* stream);
/* SSIM beside the squared error: one launch on the same inputs,
 * x = ngp_frame_sse's c and y = its gt, both float32. Wang et al. 2004 with
 * the 11 x 11 Gaussian window, sigma 1.5, g[k] = exp(-(k - 5)^2 / (2 * 1.5^2))
 * normalised to sum 1 (computed here in double and handed to the kernel),
 * applied separably over the valid region: (H - 10) x (W - 10) positions per
 * channel, no padding. Per channel and position, with E[.] the windowed mean,
 *   mux = E[x], muy = E[y], sx = E[x x] - mux mux, sy = E[y y] - muy muy,
 *   sxy = E[x y] - mux muy,
 *   ssim = ((2 mux muy + C1) (2 sxy + C2)) / ((mux mux + muy muy + C1) (sx + sy + C2)),
 *   C1 = 0.01^2, C2 = 0.03^2 (data range 1),
 * every operation from the float32 x and y on in double without contraction.
 * ssim_sum_out[pose_index] = the sum of the map's 3 (H - 10) (W - 10) values
 * (the caller divides for the mean); no other element is written. map_out
 * (nullable) [(H - 10) * (W - 10) * 3], row-major, channel last: the map; null:
 * it is never stored. The sum is deterministic in ngp_frame_sse's manner: a
 * workgroup owns tiles of 32 x 16 positions in a fixed assignment, its threads
 * add their values in a fixed order and tree, and the workgroup that finishes
 * last (an integer ticket) adds the partials in index order; no floating-point
 * atomics, the same bits from run to run for one (H, W). A non-finite x or y
 * makes the sum non-finite. Nothing outside the H x W images is read. The
 * partials and the ticket are the library's: one call at a time per device;
 * the entry clears the ticket on the stream before the launch. The caller
 * guarantees pose_index < n. Null image / weights_sum / ssim_sum_out, a bad
 * source, H * W outside [1, 2^28), H or W below 11, image or weights_sum not
 * 16-byte aligned, ssim_sum_out or map_out not 8-byte aligned: NGP_ERR_ARG. */
int ngp_frame_ssim(uint32_t H, uint32_t W, const float* image, const float* weights_sum, float bg_color,
                   const ngp_image_source* src, uint32_t pose_index, double* ssim_sum_out, double* map_out,
                   void* stream);

/* ------------------------------------------------------------------------ */
/* Background model (the reference's --bg_radius, nerf/network.py:107-129,  */
/* 202-217; nerf/renderer.py:272-277): csrc/background.hip, DESIGN.md 15     */
/* ------------------------------------------------------------------------ */

/* Bytes of the backward's fixed-point scratch (64-bit integers) for a table of
 * table_values values (entries x 2): [table_values | 3072 weight gradients].
 * 16-byte aligned; zero it once, the backward leaves it zero. */
size_t ngp_background_scratch_bytes(uint64_t table_values);
/* One launch over N rays: sph = ngp_sph_from_ray's coordinates, x = [half(SH
 * degree 4 of rays_d) (16) | the 2-D hash grid at (sph + 1) / 2, 4 levels x 2
 * features in the half arithmetic of ngp_grid_encode_forward (8) | 0 (8)],
 * bg f32 [N, 3] = sigmoid(FFMLP 32 -> 64 -> 3 (x)) with the logits and the
 * sigmoid rounded to half, as the autograd ops give them under autocast.
 *   table [entries, 2] fp32 (each value rounded to half on load) or fp16
 *     (table_dtype NGP_DTYPE_F32 / _F16), offsets i32 [5] on the device, S =
 *     log2(per_level_scale), H = base_resolution; weights fp16 [64 * 32 + 16 *
 *     64] in FFMLP's layout, 16-byte aligned.
 *   Training (rgba f32 [N, 4] non-null): rgba[n] := (rgb * a + 1 * (1 - a), 1)
 *     in fp32 without contraction, the white-blended target a background model
 *     trains against (nerf/utils.py:508-517); x_save fp16 [N, 32] and sph_save
 *     f32 [N, 2] (each nullable) keep x and (sph + 1) / 2 for the backward.
 *   Inference blend (image f32 [N, 3] and weights_sum f32 [N], both or
 *     neither): image[p] += (1 - weights_sum[p]) * bg[p].
 * Null required buffers, radius <= 0, N == 0, num_levels != 4 or level_dim != 2:
 * NGP_ERR_ARG; an MLP other than input_dim 32, hidden_dim 64, num_layers 2:
 * NGP_ERR_UNSUPPORTED; both before any device work. */
int ngp_background_forward(const float* rays_o, const float* rays_d, float radius, uint32_t N, const void* table,
                           int32_t table_dtype, const int32_t* offsets, uint32_t num_levels, uint32_t level_dim,
                           float S, uint32_t H, const void* weights, uint32_t input_dim, uint32_t hidden_dim,
                           uint32_t num_layers, float* bg, float* rgba, void* x_save, float* sph_save, float* image,
                           const float* weights_sum, void* stream);
/* Two launches after the composite (which must have written out_image [N, 3]
 * and out_ws [N]) and before the batch buffers are drawn again. Per ray n,
 * index = rays[n * 3] (rays null: n),
 *   g_bg = scale * color_weight * (2 / (3 N)) * (out_image - gt) * (1 - out_ws)
 * with scale the state's GradScaler scale and gt f32 [N, 4] the blended
 * target; then through the half sigmoid and both layers (the hidden layer is
 * recomputed from x_save): dW of both, and the input gradient of the 8 grid
 * columns, scattered with the bilinear weights at sph_save. Each wave sums dW
 * over its rays in fp32 MFMA accumulators; every sum across waves is a 64-bit
 * integer atomic add in fixed point (2^-24) into scratch, so the result does
 * not depend on the atomics' order (bit-reproducible). The second launch
 * rounds scratch to fp16 into grad_table [table_values] and grad_weights
 * [3072] and zeroes scratch. inf_flag gets 1 ORed in when a contribution is
 * not finite or a sum leaves fp16's range, i.e. whenever a value written to
 * the gradients is not finite or stands for a sum that was. Argument checks
 * as the forward's. */
int ngp_background_backward(const int32_t* rays, uint32_t N, const float* out_image, const float* out_ws,
                            const float* gt, const float* bg, const void* x_save, const float* sph_save,
                            const int32_t* offsets, uint32_t num_levels, uint32_t level_dim, float S, uint32_t H,
                            uint64_t table_values, const void* weights, uint32_t input_dim, uint32_t hidden_dim,
                            uint32_t num_layers, const void* state, float color_weight, float radius, void* scratch,
                            void* grad_table, void* grad_weights, int32_t* inf_flag, void* stream);

/* ------------------------------------------------------------------------ */
/* Baseline JPEG of a uint8 frame on the device: csrc/jpeg.hip, DESIGN.md 19 */
/* ------------------------------------------------------------------------ */

/* The worst-case size in bytes of the entropy-coded scan ngp_jpeg_encode writes
 * for an H x W image of `components` (1 or 3) components: with B = ceil(W / 8)
 * * components blocks in each of the n = ceil(H / 8) restart intervals,
 * n * (2 * (216 * B + 1) + 2). Every coefficient costs at most a 16-bit code and
 * 11 magnitude bits (a ZRL is charged to the first of its 16 zeros, the EOB to
 * the first trailing zero), so a block is at most 64 * 27 bits = 216 bytes; the
 * padding completes at most one more byte per interval, byte stuffing at most
 * doubles the bytes, and each interval but the last is followed by the 2 bytes
 * of RSTm. 0 for components outside {1, 3} or H, W outside [1, 65535]. */
size_t ngp_jpeg_scan_capacity(uint32_t H, uint32_t W, uint32_t components);
/* int16 elements of ngp_jpeg_encode's workspace: the [blocks, 64] coefficients,
 * then the library's own part (the intervals' lengths and their byte-stuffed
 * slabs of 2 * (216 * B + 1) bytes each). 0 for the arguments above. */
size_t ngp_jpeg_workspace_elems(uint32_t H, uint32_t W, uint32_t components);
/* Baseline sequential JPEG (T.81 SOF0, 8 bit) of pixels u8 [H, W, 3] (RGB) or
 * [H, W] (components 3 / 1) on the device: the entropy-coded scan, i.e. the
 * bytes between the SOS header and EOI, into out; *out_len (device) = its
 * length. Three launches on `stream`, no host synchronisation, no
 * floating-point atomics; the bytes depend on the inputs alone.
 *   - 3 components: Y, Cb, Cr by the JFIF conversion in fp32 (Y = 0.299 R +
 *     0.587 G + 0.114 B, Cb = -0.168736 R - 0.331264 G + 0.5 B + 128, Cr = 0.5 R -
 *     0.418688 G - 0.081312 B + 128, no rounding in between), all sampled 1 x 1;
 *     the MCU is one 8 x 8 block per component, Y, Cb, Cr. Level shift -128.
 *     Edge blocks repeat the last column and row.
 *   - 8 x 8 DCT-II in fp32, orthonormal (T.81 A.3.3); each coefficient divided
 *     by its quantiser (qtable_luma / qtable_chroma: HOST arrays of 64 values in
 *     natural order, each in 1..255; qtable_chroma may be null for 1 component)
 *     and rounded to nearest (a tie may go either way); DC clamped to +-2047, AC
 *     to +-1023; zigzag order of T.81 Figure A.6.
 *   - coef_ws: int16 [ngp_jpeg_workspace_elems], 16-byte aligned; its first
 *     blocks * 64 elements receive the quantised coefficients in zigzag order,
 *     block (mcu_row * ceil(W / 8) + mcu_col) * components + component.
 *   - Huffman coding with the typical tables of T.81 Annex K.3 (csrc/
 *     jpeg_tables.h). Restart interval = one MCU row (DRI = ceil(W / 8)): DC
 *     predictors reset, the last byte padded with 1 bits, RSTm (m = interval mod
 *     8) after every interval but the last, 0xFF followed by 0x00 inside.
 * capacity: the bytes of out, at least ngp_jpeg_scan_capacity (bytes past
 * capacity are never written). Null buffers, components outside {1, 3}, H or W
 * outside [1, 65535], a quantiser outside 1..255, a misaligned workspace, a
 * capacity below the bound (or a bound past 2^32): NGP_ERR_ARG before any
 * device work. */
int ngp_jpeg_encode(const uint8_t* pixels, uint32_t H, uint32_t W, uint32_t components, const uint16_t* qtable_luma,
                    const uint16_t* qtable_chroma, int16_t* coef_ws, uint8_t* out, size_t capacity, uint32_t* out_len,
                    void* stream);

/* ------------------------------------------------------------------------ */
/* Signed distance fields of triangle meshes: csrc/sdf.hip, DESIGN.md 21      */
/* ------------------------------------------------------------------------ */

#define NGP_SDF_BLOCK_FACES 64 /* faces per block of the prepared mesh (one box each) */
#define NGP_SDF_MAPE_BLOCKS 256 /* doubles of the loss's partial sums */

/* The prepared mesh (sdf/provider.py prepare_mesh): T >= 1 faces sorted by the
 * Morton code of their centroid,
 *   tris       f32 [T, 9]     the corners a, b, c;
 *   normals    f32 [T, 7, 3]  per feature code 0..6: the unit face normal, the
 *                             pseudo-normals of the edges ab, bc, ca (the sum
 *                             of the two incident face normals) and of the
 *                             vertices a, b, c (angle weighted), outwards;
 *   block_aabb f32 [ceil(T / 64), 6]  min then max of every block of 64 faces;
 *   cdf        f32 [T]        cumulative area fractions, the last one 1. */

/* One training batch of the reference's sdf/provider.py:66-75, points f32
 * [N, 3]: [0, N/2) on the surface, [N/2, 7N/8) on the surface plus 0.01 *
 * normal noise, [7N/8, N) uniform in [-1, 1)^3. Point n of step s draws
 * rng_unit(seed, s, n, stream) of the counter RNG: streams 0 1 2 the triangle
 * (the first whose cdf entry exceeds u0, at most T - 1) and the barycentrics
 * (1 - sqrt(u1), sqrt(u1) (1 - u2), sqrt(u1) u2), 3..6 the Box-Muller pairs
 * (x and y from one, z from the other); a uniform point is 2 u - 1 of streams
 * 0 1 2. s is counter[0] (device uint32[2]; [1] is the launch's own ticket and
 * is left 0); the launch leaves counter[0] = s + 1, so no step needs a host
 * value. tri (nullable) int32 [N]: the source triangle, -1 for a uniform
 * point. N % 8 != 0: NGP_ERR_ARG before any launch; N == 0: NGP_OK. */
int ngp_sdf_sample(const float* tris, const float* cdf, uint32_t T, uint32_t N, uint32_t seed, uint32_t* counter,
                   float* points, int32_t* tri, void* stream);

/* Exact signed distance of n points f32 [n, 3] to the prepared mesh, negative
 * inside (the reference's -sdf_fn(points)): the minimum over all faces of the
 * point-to-triangle distance, signed by (p - q) . n_feature of the closest
 * feature; ties keep the face met first. tri (nullable) int32 [n]: a face in
 * [0, T) whose distance starts the point's search (anything else: no start).
 * feature (nullable) int32 [n]: face * 8 + code. cull != 0 skips a block of
 * faces whose box is farther from every point of a wave than the point's best
 * distance, with a margin over the rounding of both; the results are the plain
 * scan's bit for bit. n == 0: NGP_OK without a launch. */
int ngp_sdf_query(const float* points, uint32_t n, const float* tris, const float* normals, const float* block_aabb,
                  uint32_t T, const int32_t* tri, int32_t cull, float* sdf, int32_t* feature, void* stream);

/* The reference's loss.py mape_loss over n elements: *loss (device double) =
 * mean(|pred - y| / (|y| + 1e-2)), every term in float64, summed in a fixed
 * order through partials (device double[NGP_SDF_MAPE_BLOCKS]). grad
 * (nullable, pred's dtype): sign(pred - y) / ((|y| + 1e-2) n) evaluated as
 * torch's fp32 backward of that formula does, (1 / n) / (|y| + 0.01f) *
 * sign, times *grad_scale (device float, nullable) before the rounding to
 * pred's dtype. pred_dtype NGP_DTYPE_F32 or NGP_DTYPE_F16; n in [1, 2^24). */
int ngp_sdf_mape(const void* pred, int32_t pred_dtype, const float* y, uint64_t n, const float* grad_scale, void* grad,
                 double* partials, double* loss, void* stream);

/* ------------------------------------------------------------------------ */
/* TensoRF's vector-matrix decomposition: csrc/tensorf.hip, DESIGN.md 22      */
/* ------------------------------------------------------------------------ */

#define NGP_VM_MAX_RES 4096  /* texels per axis */
#define NGP_VM_MAX_RANK 1024 /* components per plane / line */
#define NGP_VM_FIXED_BITS 32 /* the backward's quantum: 2^-32 of the power of two above max |g| */

/* One set of the decomposition: component i is plane[i] f32 [H, W, rank[i]]
 * times line[i] f32 [D, rank[i]], with W = res[m0], H = res[m1], (m0, m1) =
 * (0,1) (0,2) (1,2) and D = res[v], v = 2 1 0, for i = 0 1 2. */
typedef struct ngp_vm_set {
    const float* plane[3];
    const float* line[3];
    uint32_t rank[3];
} ngp_vm_set;

/* x f32 [N, 3] in world units, aabb6 (device) f32 [6]: c = 2 * (x - lo) / (hi -
 * lo) - 1 in float32 in that order, then every plane at (c[m0], c[m1]) and
 * every line at c[v] as grid_sample(mode='bilinear', padding_mode='zeros',
 * align_corners=True) samples them (a texel outside the texture counts as
 * zero). sum_set (nullable): sigma_feat f32 [N] = sum_i sum_r plane_i[r] *
 * line_i[r]. cat_set (nullable): prod f32 [N, sum_i rank_i], the products,
 * component-major. N == 0: NGP_OK without a launch; N < 2^30. */
int ngp_vm_forward(const float* x, uint32_t N, const float* aabb6, uint32_t res0, uint32_t res1, uint32_t res2,
                   const ngp_vm_set* sum_set, float* sigma_feat, const ngp_vm_set* cat_set, float* prod, void* stream);

/* The gradient values of the sets given (nullable each): per set, sum_set
 * first, the planes 0 1 2 then the lines 0 1 2, each in its parameter's
 * layout; and the bytes of the backward's scratch for them. 0: bad arguments. */
size_t ngp_vm_grad_values(uint32_t res0, uint32_t res1, uint32_t res2, const ngp_vm_set* sum_set,
                          const ngp_vm_set* cat_set);
size_t ngp_vm_backward_scratch_bytes(uint32_t res0, uint32_t res1, uint32_t res2, const ngp_vm_set* sum_set,
                                     const ngp_vm_set* cat_set);

/* grads f32 [ngp_vm_grad_values] = the gradients of every plane and line of
 * the sets given, from grad_sigma_feat f32 [N] and / or grad_prod f32 [N, sum
 * rank] (nullable each: that set's gradients are zero); the interpolation is
 * recomputed from x. There is no gradient to x. Every contribution is rounded
 * to the nearest multiple of the quantum q = 2^(E - NGP_VM_FIXED_BITS), 2^E
 * the smallest power of two above the largest |g| of both gradients, and
 * summed in 64-bit integers: the result does not depend on the order of the
 * additions, and an entry with K contributions is within K q / 2 of the exact
 * sum of its float32 contributions. A gradient that is not finite, or a
 * contribution of 2^40 quanta or more (a weight times a parameter of 256 or
 * more times the largest g), makes every value of grads NaN. scratch: the
 * launcher clears it. N <= 2^22. */
int ngp_vm_backward(const float* x, uint32_t N, const float* aabb6, uint32_t res0, uint32_t res1, uint32_t res2,
                    const ngp_vm_set* sum_set, const float* grad_sigma_feat, const ngp_vm_set* cat_set,
                    const float* grad_prod, void* scratch, size_t scratch_bytes, float* grads, void* stream);

/* ------------------------------------------------------------------------ */
/* D-NeRF: the time-sliced density grid and the deformation network's input  */
/* row: csrc/dnerf.hip, DESIGN.md 23                                          */
/* ------------------------------------------------------------------------ */

/* Grid shape of every entry below: 1 <= T <= 1024 time slices, 1 <= C <= 16
 * cascades, H a power of two in [2, 1024], T * C * H^3 < 2^32; NGP_ERR_ARG
 * otherwise, before any device work. grid f32 [T, C, H^3]: a cell's flat index
 * is (t * C + c) * H^3 + morton3D(cell). */

#define NGP_DNERF_ENCODE_COLS 76 /* 3 + 3 * 2 * 10 columns of x, then 1 + 2 * 6 of t */

/* out [N, NGP_DNERF_ENCODE_COLS] with rows row_stride elements apart (>= the
 * columns; the elements past a row's columns are not written), out_dtype
 * NGP_DTYPE_F32 or NGP_DTYPE_F16: the frequency encoding of x f32 [N, 3] with
 * 10 octaves, then that of the time with 6, in ngp_freq_encode_forward's
 * column order (the input, then per octave f the sines of 2^f * input, then
 * the cosines), with accurate sinf / cosf. t f32: one value for every row
 * (t_stride 0) or one per row (t_stride 1). N == 0: NGP_OK without a launch;
 * N * 76 < 2^32. */
int ngp_dnerf_encode(const float* x, const float* t, uint32_t t_stride, uint32_t N, void* out, int32_t out_dtype,
                     uint32_t row_stride, void* stream);

/* The query points [lo, hi) of update number `update` of the time-sliced
 * grid: xyzs f32 [hi - lo, 3], times f32 [hi - lo], indices i32 [hi - lo]
 * (flat cell indices), a pure function of (seed, update, point) through the
 * counter RNG in a domain of its own (and, for partial updates, of the grid).
 * Points are numbered slice-major, then cascade. partial == 0: every cell,
 * point p is cell p (the grid is not read; grid, ws may be null). partial != 0:
 * per slice and cascade N = H^3 / 4 uniformly drawn cells, then N cells drawn
 * i.i.d. with replacement from that slice and cascade's occupied cells
 * (grid > 0), or uniformly where it has none; ws: the occupied lists, of
 * ngp_dnerf_grid_points_workspace_bytes(T, C, H) bytes (0: bad shape).
 * Position: (2 c / (H - 1) - 1) * (bound_c - hgs) + (2 u - 1) * hgs, bound_c =
 * min(2^c, bound), hgs = bound_c / H, with the fp32 operations of
 * ngp_density_grid_points. Time: (t + 0.5) / T + (2 u - 1) * 0.5 / T, drawn per
 * point, kept inside [float(t) / float(T), float(t + 1) / float(T)].
 * hi == lo: NGP_OK without a launch. */
size_t ngp_dnerf_grid_points_workspace_bytes(uint32_t T, uint32_t C, uint32_t H);
int ngp_dnerf_grid_points(const float* grid, uint32_t T, uint32_t C, uint32_t H, float bound, uint32_t partial,
                          uint32_t seed, uint32_t update, uint32_t lo, uint32_t hi, void* ws, size_t ws_bytes,
                          float* xyzs, float* times, int32_t* indices, void* stream);

/* ngp_density_grid_ema_pack over every slice: where grid >= 0 and tmp_grid >=
 * 0, grid = max(grid * decay, tmp_grid); tmp_grid reset to -1; stats[0] = the
 * sum of clamp(grid, 0) over all T * C * H^3 cells in double, added in a fixed
 * order without atomics (stats: NGP_DNERF_STATS_LEN doubles); bitfield u8 [T,
 * C * H^3 / 8] at min(mean_density, density_thresh), mean_density =
 * float(stats[0] / (T * C * H^3)): the mean over the whole grid, not a
 * slice's. A NaN mean clears every bit. grid 16-byte aligned. Two launches. */
#define NGP_DNERF_STATS_LEN 1025
int ngp_dnerf_grid_ema_pack(float* grid, float* tmp_grid, uint32_t T, uint32_t C, uint32_t H, float decay,
                            double density_thresh, double* stats, uint8_t* bitfield, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* NGP_HIP_H */
