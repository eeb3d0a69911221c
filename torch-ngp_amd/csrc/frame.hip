// Whole frames around the device-driven render loop (raymarching.hip,
// nerf/fused_render.py): the reference's test render (Trainer.test /
// test_step, nerf/utils.py:656-685, 743-796) renders every ray of a pose,
// quantises colour and depth to uint8 and writes PNGs. DESIGN.md §14.
//
//   k_frame_begin   one launch before the loop: the rays of all H * W pixels of
//                   one pose of a device pose stack (get_rays with N = -1,
//                   utils.py:52-136, through ngp_head::pixel_ray, the training
//                   draw's arithmetic), their near / far (ngp_head::near_far),
//                   zeroed noises, and everything ngp_render_init initialises
//   k_frame_finish  one launch after it: background blend, depth
//                   normalisation and the uint8 quantisation
//   k_frame_sse     or, in its place, the validation pass: the blended colour
//                   against the view's ground-truth image, the squared error
//                   summed in double on the device
//   k_frame_ssim    beside it, on the same two images: their SSIM, the 11 x 11
//                   Gaussian window in double through LDS tiles
//
// All but the last make one pass over the pixels and are bound by memory. A
// thread owns 4 consecutive pixels, so every [N] array moves as one 16-byte
// access per thread, every [N, 3] array as three, the 12 colour bytes as three
// dwords and the 4 depth bytes as one. The last N % 4 pixels of a frame go
// element by element (one thread).
#include "ngp_common.h"
#include "ngp_head.h"
#include "ngp_render.h"

#include <cmath>

namespace {

using ngp_render::RenderSlot;

constexpr uint32_t kThreads = 256;
constexpr uint32_t kPix = 4;  // pixels per thread

// K floats of a thread's run starting at dst / src (16-byte aligned when
// `full`): K / 4 vector accesses, or the first `live` elements one by one.
template <int K> NGP_DEV void put(float* dst, const float (&v)[K], bool full, uint32_t live) {
    if (full) {
#pragma unroll
        for (int q = 0; q < K / 4; ++q)
            reinterpret_cast<float4*>(dst)[q] = make_float4(v[q * 4], v[q * 4 + 1], v[q * 4 + 2], v[q * 4 + 3]);
    } else {
#pragma unroll
        for (int k = 0; k < K; ++k)
            if ((uint32_t)k < live) dst[k] = v[k];
    }
}
template <int K> NGP_DEV void get(const float* __restrict__ src, float (&v)[K], bool full, uint32_t live) {
    if (full) {
#pragma unroll
        for (int q = 0; q < K / 4; ++q) {
            const float4 t = reinterpret_cast<const float4*>(src)[q];
            v[q * 4] = t.x; v[q * 4 + 1] = t.y; v[q * 4 + 2] = t.z; v[q * 4 + 3] = t.w;
        }
    } else {
#pragma unroll
        for (int k = 0; k < K; ++k) v[k] = (uint32_t)k < live ? src[k] : 0.0f;
    }
}

struct FrameCamera {
    float fx, fy, cx, cy;
    uint32_t W, N;  // N = H * W
    float aabb[6];
    float min_near;
};

struct FrameRays {
    float *rays_o, *rays_d, *nears, *fars, *noises, *rays_t, *weights_sum, *depth, *image;
    int32_t* rays_alive;
    RenderSlot* state;
};

__global__ void __launch_bounds__(kThreads)
k_frame_begin(const float* __restrict__ pose, FrameCamera cam, FrameRays out) {
    const uint32_t g = blockIdx.x * kThreads + threadIdx.x;
    const uint32_t p0 = g * kPix;
    if (g == 0) {  // ngp_render_init's loop state
        out.state[0] = RenderSlot{0, (int32_t)cam.N, 0, 0};
        out.state[1] = RenderSlot{0, 0, 0, 0};
    }
    if (p0 >= cam.N) return;
    const uint32_t cnt = min(kPix, cam.N - p0);
    const bool full = cnt == kPix;
    float ro[kPix * 3], rd[kPix * 3], nr[kPix], fr[kPix], alive[kPix];
    const float zero1[kPix] = {}, zero3[kPix * 3] = {};
#pragma unroll
    for (uint32_t k = 0; k < kPix; ++k) {
        // (pixels past the frame, in the tail's thread only, are computed and not stored)
        const uint32_t pix = min(p0 + k, cam.N - 1u);
        float o[3], d[3];
        ngp_head::pixel_ray(pix, cam.W, cam.fx, cam.fy, cam.cx, cam.cy, pose, o, d);
        ngp_head::near_far(o, d, cam.aabb, cam.min_near, nr[k], fr[k]);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            ro[k * 3 + c] = o[c];
            rd[k * 3 + c] = d[c];
        }
        alive[k] = __int_as_float((int32_t)(p0 + k));
    }
    put(out.rays_o + (size_t)p0 * 3, ro, full, cnt * 3);
    put(out.rays_d + (size_t)p0 * 3, rd, full, cnt * 3);
    put(out.nears + p0, nr, full, cnt);
    put(out.fars + p0, fr, full, cnt);
    put(out.rays_t + p0, nr, full, cnt);  // the march starts at near
    put(reinterpret_cast<float*>(out.rays_alive) + p0, alive, full, cnt);  // alive list 0 = arange(N)
    put(out.noises + p0, zero1, full, cnt);  // perturb = False
    put(out.weights_sum + p0, zero1, full, cnt);
    put(out.depth + p0, zero1, full, cnt);
    put(out.image + (size_t)p0 * 3, zero3, full, cnt * 3);
}

// The reference's (x * 255).astype(np.uint8) (utils.py:776, :779) made total:
// x clamped to [0, 1], truncated; a non-finite x gives 0.
NGP_DEV uint32_t quantise(float x) {
    if (!(fabsf(x) < INFINITY)) return 0u;
    return (uint32_t)(fminf(fmaxf(x, 0.0f), 1.0f) * 255.0f);
}

__global__ void __launch_bounds__(kThreads)
k_frame_finish(uint32_t N, const float* __restrict__ image, const float* __restrict__ weights_sum,
               const float* __restrict__ depth, const float* __restrict__ nears, const float* __restrict__ fars,
               float bg, uint8_t* __restrict__ rgb8, uint8_t* __restrict__ depth8, float* __restrict__ image_out,
               float* __restrict__ depth_out) {
    const uint32_t p0 = (blockIdx.x * kThreads + threadIdx.x) * kPix;
    if (p0 >= N) return;
    const uint32_t cnt = min(kPix, N - p0);
    const bool full = cnt == kPix;
    float im[kPix * 3], ws[kPix], dp[kPix], nr[kPix], fr[kPix];
    get(image + (size_t)p0 * 3, im, full, cnt * 3);
    get(weights_sum + p0, ws, full, cnt);
    get(depth + p0, dp, full, cnt);
    get(nears + p0, nr, full, cnt);
    get(fars + p0, fr, full, cnt);
    float c[kPix * 3], z[kPix];
    uint32_t cq[kPix * 3], zq[kPix];
#pragma unroll
    for (uint32_t k = 0; k < kPix; ++k) {
        // FusedRenderer.render: image + (1 - weights_sum) * bg_color,
        // clamp(depth - nears, min=0) / (fars - nears), operation for operation
        const float w = (1.0f - ws[k]) * bg;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            c[k * 3 + j] = im[k * 3 + j] + w;
            cq[k * 3 + j] = quantise(c[k * 3 + j]);
        }
        const float t = dp[k] - nr[k];
        z[k] = (t < 0.0f ? 0.0f : t) / (fr[k] - nr[k]);  // torch.clamp keeps a NaN; near == far (a miss): 0 / 0
        zq[k] = quantise(z[k]);
    }
    if (full) {
        uint32_t* rgb = reinterpret_cast<uint32_t*>(rgb8 + (size_t)p0 * 3);
#pragma unroll
        for (int q = 0; q < 3; ++q)
            rgb[q] = cq[q * 4] | (cq[q * 4 + 1] << 8) | (cq[q * 4 + 2] << 16) | (cq[q * 4 + 3] << 24);
        *reinterpret_cast<uint32_t*>(depth8 + p0) = zq[0] | (zq[1] << 8) | (zq[2] << 16) | (zq[3] << 24);
    } else {
#pragma unroll
        for (uint32_t k = 0; k < kPix; ++k) {
            if (k >= cnt) break;
#pragma unroll
            for (int j = 0; j < 3; ++j) rgb8[(size_t)(p0 + k) * 3 + j] = (uint8_t)cq[k * 3 + j];
            depth8[p0 + k] = (uint8_t)zq[k];
        }
    }
    if (image_out) put(image_out + (size_t)p0 * 3, c, full, cnt * 3);
    if (depth_out) put(depth_out + p0, z, full, cnt);
}

// The validation pass: the squared error of a rendered view
// against its ground-truth image, summed on the device. A workgroup's threads
// take 4-pixel runs in a grid-stride loop, each thread adds its squares up in
// double in pixel order, the workgroup adds its threads' sums in a fixed tree
// and stores one partial; the workgroup that finishes last (an integer ticket)
// adds the partials in index order. Nothing in the sum depends on timing, so
// it is the same from run to run. The partials and the ticket are the
// library's own (one pass at a time per device: calls are issued in stream
// order on one stream); the entry clears the ticket on the stream before every
// launch, so a pass does not depend on how an earlier one ended.
constexpr uint32_t kSseMaxBlocks = 1024;
__device__ double g_sse_partial[kSseMaxBlocks];
__device__ uint32_t g_sse_ticket;

struct GroundTruth {
    const void* pixels;  // [n_poses, H, W, channels], already offset to the pose
    uint32_t channels;
    int32_t dtype;
};

// Pixel p of the view as nerf.eval.ground_truth gives it: ngp_head::image_target's
// decode (uint8: v / 255, a true division; float32 as stored), RGBA blended on
// white, rgb * a + (1 - a), in float32.
NGP_DEV void ground_truth(const GroundTruth& gt, uint32_t p, float (&c)[3]) {
    float a = 1.0f;
    if (gt.dtype == NGP_DTYPE_U8) {
        uint32_t c0, c1, c2, c3 = 255u;
        if (gt.channels == 4) {
            const uint32_t w = static_cast<const uint32_t*>(gt.pixels)[p];
            c0 = w & 255u; c1 = (w >> 8) & 255u; c2 = (w >> 16) & 255u; c3 = w >> 24;
        } else {
            const uint8_t* q = static_cast<const uint8_t*>(gt.pixels) + (size_t)p * 3;
            c0 = q[0]; c1 = q[1]; c2 = q[2];
        }
        c[0] = (float)c0 / 255.0f; c[1] = (float)c1 / 255.0f; c[2] = (float)c2 / 255.0f;
        if (gt.channels == 4) a = (float)c3 / 255.0f;
    } else if (gt.channels == 4) {
        const float4 v = static_cast<const float4*>(gt.pixels)[p];
        c[0] = v.x; c[1] = v.y; c[2] = v.z; a = v.w;
    } else {
        const float* q = static_cast<const float*>(gt.pixels) + (size_t)p * 3;
        c[0] = q[0]; c[1] = q[1]; c[2] = q[2];
    }
    if (gt.channels == 4) {
        const float w = 1.0f - a;
#pragma unroll
        for (int j = 0; j < 3; ++j) c[j] = c[j] * a + w;
    }
}

__global__ void __launch_bounds__(kThreads)
k_frame_sse(uint32_t N, const float* __restrict__ image, const float* __restrict__ weights_sum, float bg,
            GroundTruth gt, double* __restrict__ sse_out) {
    __shared__ double s_sum[kThreads];
    __shared__ uint32_t s_last;
    double acc = 0.0;
    const uint32_t stride = gridDim.x * kThreads * kPix;
    for (uint32_t p0 = (blockIdx.x * kThreads + threadIdx.x) * kPix; p0 < N; p0 += stride) {
        const uint32_t cnt = min(kPix, N - p0);
        const bool full = cnt == kPix;
        float im[kPix * 3], ws[kPix];
        get(image + (size_t)p0 * 3, im, full, cnt * 3);
        get(weights_sum + p0, ws, full, cnt);
#pragma unroll
        for (uint32_t k = 0; k < kPix; ++k) {
            if (k >= cnt) break;
            float t[3];
            ground_truth(gt, p0 + k, t);
            const float w = (1.0f - ws[k]) * bg;  // k_frame_finish's blend
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const float d = (im[k * 3 + j] + w) - t[j];
                acc += (double)(d * d);
            }
        }
    }
    s_sum[threadIdx.x] = acc;
    __syncthreads();
    for (uint32_t o = kThreads / 2; o > 0; o >>= 1) {
        if (threadIdx.x < o) s_sum[threadIdx.x] += s_sum[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        __hip_atomic_store(&g_sse_partial[blockIdx.x], s_sum[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __threadfence();
        s_last = atomicAdd(&g_sse_ticket, 1u) == gridDim.x - 1u;
    }
    __syncthreads();
    if (!s_last) return;
    __threadfence();
    // the last workgroup: partial b to thread b % 256 in ascending b, then the same tree
    acc = 0.0;
    for (uint32_t b = threadIdx.x; b < gridDim.x; b += kThreads)
        acc += __hip_atomic_load(&g_sse_partial[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_sum[threadIdx.x] = acc;
    __syncthreads();
    for (uint32_t o = kThreads / 2; o > 0; o >>= 1) {
        if (threadIdx.x < o) s_sum[threadIdx.x] += s_sum[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) *sse_out = s_sum[0];
}

// SSIM of a rendered view against its ground-truth image: the
// 11 x 11 Gaussian window (sigma 1.5) of Wang et al. 2004 applied separably
// over the valid region, (H - 10) x (W - 10) positions per channel, on the two
// float32 images k_frame_sse compares; every operation from those values on is
// in double (the variances cancel against C2 = 8.1e-4). A workgroup owns tiles
// of kSsimTileW x kSsimTileH positions: it stages a tile's pixels and the
// 10-pixel halo of both images (blend and decode done here, zeros past the
// image), then per channel runs the horizontal pass of the five moments into
// LDS and the vertical pass and the formula from there. Thread t owns column
// t % 32 and rows t / 32 and t / 32 + 8 of a tile and adds its values up in
// tile, channel, row order; workgroups take tiles b, b + gridDim.x, ...; the
// sum over threads and workgroups is k_frame_sse's (tree, ticket, partials in
// index order), so it depends on (H, W) alone.
constexpr uint32_t kSsimWin = 11, kSsimHalo = kSsimWin - 1;
constexpr uint32_t kSsimTileW = 32, kSsimTileH = 16;
constexpr uint32_t kSsimInW = kSsimTileW + kSsimHalo, kSsimInH = kSsimTileH + kSsimHalo;  // 42 x 26 staged pixels
constexpr uint32_t kSsimMaxBlocks = 1024;
static_assert(kSsimTileW * kSsimTileH == 2 * kThreads, "a thread owns two positions of a tile");
__device__ double g_ssim_partial[kSsimMaxBlocks];
__device__ uint32_t g_ssim_ticket;

struct SsimWindow {
    double g[kSsimWin];  // the normalised 1-D weights, the host's
};

__global__ void __launch_bounds__(kThreads)
k_frame_ssim(uint32_t H, uint32_t W, const float* __restrict__ image, const float* __restrict__ weights_sum, float bg,
             GroundTruth gt, SsimWindow win, uint32_t tiles_x, uint32_t n_tiles, double* __restrict__ map_out,
             double* __restrict__ ssim_out) {
    __shared__ float s_in[2][3][kSsimInH][kSsimInW];         // [x | y][channel]: 26,208 bytes
    __shared__ double s_h[5][kSsimInH][kSsimTileW];          // one channel's horizontal pass: 33,280 bytes
    __shared__ double s_sum[kThreads];
    __shared__ uint32_t s_last;
    const double C1 = 0.01 * 0.01, C2 = 0.03 * 0.03;
    const uint32_t oh = H - kSsimHalo, ow = W - kSsimHalo;   // the map's extent
    const uint32_t tc = threadIdx.x % kSsimTileW, tr = threadIdx.x / kSsimTileW;
    double acc = 0.0;
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint32_t y0 = tile / tiles_x * kSsimTileH, x0 = tile % tiles_x * kSsimTileW;
        for (uint32_t i = threadIdx.x; i < kSsimInH * kSsimInW; i += kThreads) {
            const uint32_t r = i / kSsimInW, c = i % kSsimInW;
            float xv[3] = {0.0f, 0.0f, 0.0f}, yv[3] = {0.0f, 0.0f, 0.0f};
            if (y0 + r < H && x0 + c < W) {  // (only the last tile row / column's positions past the map need the rest)
                const uint32_t p = (y0 + r) * W + (x0 + c);
                const float w = (1.0f - weights_sum[p]) * bg;  // k_frame_finish's blend
#pragma unroll
                for (int j = 0; j < 3; ++j) xv[j] = image[(size_t)p * 3 + j] + w;
                ground_truth(gt, p, yv);
            }
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                s_in[0][j][r][c] = xv[j];
                s_in[1][j][r][c] = yv[j];
            }
        }
        __syncthreads();
        for (uint32_t ch = 0; ch < 3; ++ch) {
            for (uint32_t i = threadIdx.x; i < kSsimInH * kSsimTileW; i += kThreads) {
                const uint32_t r = i / kSsimTileW, c = i % kSsimTileW;
                double m[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (uint32_t k = 0; k < kSsimWin; ++k) {
                    const double x = (double)s_in[0][ch][r][c + k], y = (double)s_in[1][ch][r][c + k], g = win.g[k];
                    m[0] += g * x;
                    m[1] += g * y;
                    m[2] += g * (x * x);
                    m[3] += g * (y * y);
                    m[4] += g * (x * y);
                }
#pragma unroll
                for (int q = 0; q < 5; ++q) s_h[q][r][c] = m[q];
            }
            __syncthreads();
#pragma unroll
            for (uint32_t half = 0; half < 2; ++half) {
                const uint32_t r = tr + half * (kSsimTileH / 2);
                double m[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (uint32_t k = 0; k < kSsimWin; ++k)
#pragma unroll
                    for (int q = 0; q < 5; ++q) m[q] += win.g[k] * s_h[q][r + k][tc];
                const double mux = m[0], muy = m[1];
                const double sx = m[2] - mux * mux, sy = m[3] - muy * muy, sxy = m[4] - mux * muy;
                const double v = ((2.0 * mux * muy + C1) * (2.0 * sxy + C2)) /
                                 ((mux * mux + muy * muy + C1) * (sx + sy + C2));
                if (y0 + r < oh && x0 + tc < ow) {
                    acc += v;
                    if (map_out) map_out[((size_t)(y0 + r) * ow + (x0 + tc)) * 3 + ch] = v;
                }
            }
            __syncthreads();  // s_h, and after the last channel s_in, are written again
        }
    }
    s_sum[threadIdx.x] = acc;
    __syncthreads();
    for (uint32_t o = kThreads / 2; o > 0; o >>= 1) {
        if (threadIdx.x < o) s_sum[threadIdx.x] += s_sum[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        __hip_atomic_store(&g_ssim_partial[blockIdx.x], s_sum[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __threadfence();
        s_last = atomicAdd(&g_ssim_ticket, 1u) == gridDim.x - 1u;
    }
    __syncthreads();
    if (!s_last) return;
    __threadfence();
    // the last workgroup: partial b to thread b % 256 in ascending b, then the same tree
    acc = 0.0;
    for (uint32_t b = threadIdx.x; b < gridDim.x; b += kThreads)
        acc += __hip_atomic_load(&g_ssim_partial[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_sum[threadIdx.x] = acc;
    __syncthreads();
    for (uint32_t o = kThreads / 2; o > 0; o >>= 1) {
        if (threadIdx.x < o) s_sum[threadIdx.x] += s_sum[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) *ssim_out = s_sum[0];
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

int check_frame_size(uint32_t H, uint32_t W, const char* who) {
    NGP_REQUIRE(H >= 1 && W >= 1 && (uint64_t)H * W <= 0x7fffffffu / 8u, NGP_ERR_ARG,
                "%s: H * W must be in [1, 2^28), got %u x %u", who, H, W);
    return NGP_OK;
}

}  // namespace

extern "C" int ngp_frame_begin(const float* poses, uint32_t n_poses, uint32_t pose_index, const float* intrinsics4,
                               uint32_t H, uint32_t W, const float* aabb6, float min_near, float* rays_o,
                               float* rays_d, float* nears, float* fars, float* noises, int32_t* rays_alive,
                               float* rays_t, float* weights_sum, float* depth, float* image, void* state,
                               void* stream) {
    if (int e = check_frame_size(H, W, "frame_begin")) return e;
    NGP_REQUIRE(poses && intrinsics4 && aabb6 && state && rays_o && rays_d && nears && fars && noises &&
                    rays_alive && rays_t && weights_sum && depth && image,
                NGP_ERR_ARG, "frame_begin: null buffer");
    NGP_REQUIRE(pose_index < n_poses, NGP_ERR_ARG, "frame_begin: pose %u of a stack of %u", pose_index, n_poses);
    NGP_REQUIRE(aligned16(rays_o) && aligned16(rays_d) && aligned16(nears) && aligned16(fars) && aligned16(noises) &&
                    aligned16(rays_alive) && aligned16(rays_t) && aligned16(weights_sum) && aligned16(depth) &&
                    aligned16(image) && aligned16(state),
                NGP_ERR_ARG, "frame_begin: the ray buffers must be 16-byte aligned");
    FrameCamera cam;
    cam.fx = intrinsics4[0]; cam.fy = intrinsics4[1]; cam.cx = intrinsics4[2]; cam.cy = intrinsics4[3];
    cam.W = W;
    cam.N = H * W;
    for (int k = 0; k < 6; ++k) cam.aabb[k] = aabb6[k];
    cam.min_near = min_near;
    const FrameRays out{rays_o, rays_d, nears, fars, noises, rays_t, weights_sum, depth, image, rays_alive,
                        static_cast<RenderSlot*>(state)};
    k_frame_begin<<<ngp_div_up(ngp_div_up(cam.N, kPix), kThreads), kThreads, 0, ngp_stream(stream)>>>(
        poses + (size_t)pose_index * 16, cam, out);
    return ngp_check_launch("frame_begin");
}

extern "C" int ngp_frame_finish(uint32_t H, uint32_t W, const float* image, const float* weights_sum,
                                const float* depth, const float* nears, const float* fars, float bg_color,
                                uint8_t* rgb8, uint8_t* depth8, float* image_out, float* depth_out, void* stream) {
    if (int e = check_frame_size(H, W, "frame_finish")) return e;
    NGP_REQUIRE(image && weights_sum && depth && nears && fars && rgb8 && depth8, NGP_ERR_ARG,
                "frame_finish: null buffer");
    NGP_REQUIRE(aligned16(image) && aligned16(weights_sum) && aligned16(depth) && aligned16(nears) &&
                    aligned16(fars) && aligned16(image_out) && aligned16(depth_out) &&
                    (reinterpret_cast<uintptr_t>(rgb8) & 3u) == 0 && (reinterpret_cast<uintptr_t>(depth8) & 3u) == 0,
                NGP_ERR_ARG, "frame_finish: float buffers must be 16-byte aligned, uint8 outputs 4-byte aligned");
    const uint32_t N = H * W;
    k_frame_finish<<<ngp_div_up(ngp_div_up(N, kPix), kThreads), kThreads, 0, ngp_stream(stream)>>>(
        N, image, weights_sum, depth, nears, fars, bg_color, rgb8, depth8, image_out, depth_out);
    return ngp_check_launch("frame_finish");
}

extern "C" int ngp_frame_sse(uint32_t H, uint32_t W, const float* image, const float* weights_sum, float bg_color,
                             const ngp_image_source* src, uint32_t pose_index, double* sse_out, void* stream) {
    if (int e = check_frame_size(H, W, "frame_sse")) return e;
    if (int e = ngp_head::check_image_source(src, "frame_sse")) return e;
    NGP_REQUIRE(image && weights_sum && sse_out, NGP_ERR_ARG, "frame_sse: null buffer");
    NGP_REQUIRE(aligned16(image) && aligned16(weights_sum) && (reinterpret_cast<uintptr_t>(sse_out) & 7u) == 0,
                NGP_ERR_ARG, "frame_sse: float buffers must be 16-byte aligned, sse_out 8-byte aligned");
    const uint32_t N = H * W;
    const size_t px_bytes = (size_t)src->channels * (src->dtype == NGP_DTYPE_F32 ? 4 : 1);
    const GroundTruth gt{static_cast<const char*>(src->pixels) + (size_t)pose_index * N * px_bytes, src->channels,
                         src->dtype};
    const uint32_t want = ngp_div_up(ngp_div_up(N, kPix), kThreads);
    const uint32_t blocks = want < kSseMaxBlocks ? want : kSseMaxBlocks;  // a function of N alone: the sum's order
    // the ticket starts at 0 whatever an earlier pass left (one that was aborted, say)
    void* ticket = nullptr;
    NGP_REQUIRE(hipGetSymbolAddress(&ticket, HIP_SYMBOL(g_sse_ticket)) == hipSuccess &&
                    hipMemsetAsync(ticket, 0, sizeof(uint32_t), ngp_stream(stream)) == hipSuccess,
                NGP_ERR_HIP, "frame_sse: could not clear the ticket");
    k_frame_sse<<<blocks, kThreads, 0, ngp_stream(stream)>>>(N, image, weights_sum, bg_color, gt,
                                                             sse_out + pose_index);
    return ngp_check_launch("frame_sse");
}

extern "C" int ngp_frame_ssim(uint32_t H, uint32_t W, const float* image, const float* weights_sum, float bg_color,
                              const ngp_image_source* src, uint32_t pose_index, double* ssim_sum_out,
                              double* map_out, void* stream) {
    if (int e = check_frame_size(H, W, "frame_ssim")) return e;
    if (int e = ngp_head::check_image_source(src, "frame_ssim")) return e;
    NGP_REQUIRE(image && weights_sum && ssim_sum_out, NGP_ERR_ARG, "frame_ssim: null buffer");
    NGP_REQUIRE(aligned16(image) && aligned16(weights_sum) &&
                    (reinterpret_cast<uintptr_t>(ssim_sum_out) & 7u) == 0 &&
                    (reinterpret_cast<uintptr_t>(map_out) & 7u) == 0,
                NGP_ERR_ARG, "frame_ssim: float buffers must be 16-byte aligned, ssim_sum_out and map_out 8-byte aligned");
    NGP_REQUIRE(H >= kSsimWin && W >= kSsimWin, NGP_ERR_ARG,
                "frame_ssim: the 11 x 11 window needs H, W >= 11, got %u x %u", H, W);
    const uint32_t N = H * W;
    const size_t px_bytes = (size_t)src->channels * (src->dtype == NGP_DTYPE_F32 ? 4 : 1);
    const GroundTruth gt{static_cast<const char*>(src->pixels) + (size_t)pose_index * N * px_bytes, src->channels,
                         src->dtype};
    // g[k] = exp(-(k - 5)^2 / (2 * 1.5^2)), normalised to sum 1 (added in ascending k)
    SsimWindow win;
    double total = 0.0;
    for (uint32_t k = 0; k < kSsimWin; ++k) {
        const double d = (double)k - 5.0;
        win.g[k] = std::exp(-(d * d) / (2.0 * 1.5 * 1.5));
        total += win.g[k];
    }
    for (uint32_t k = 0; k < kSsimWin; ++k) win.g[k] /= total;
    const uint32_t tiles_x = ngp_div_up(W - kSsimHalo, kSsimTileW), tiles_y = ngp_div_up(H - kSsimHalo, kSsimTileH);
    const uint32_t n_tiles = tiles_x * tiles_y;
    const uint32_t blocks = n_tiles < kSsimMaxBlocks ? n_tiles : kSsimMaxBlocks;  // a function of (H, W) alone
    // the ticket starts at 0 whatever an earlier pass left (one that was aborted, say)
    void* ticket = nullptr;
    NGP_REQUIRE(hipGetSymbolAddress(&ticket, HIP_SYMBOL(g_ssim_ticket)) == hipSuccess &&
                    hipMemsetAsync(ticket, 0, sizeof(uint32_t), ngp_stream(stream)) == hipSuccess,
                NGP_ERR_HIP, "frame_ssim: could not clear the ticket");
    k_frame_ssim<<<blocks, kThreads, 0, ngp_stream(stream)>>>(H, W, image, weights_sum, bg_color, gt, win, tiles_x,
                                                              n_tiles, map_out, ssim_sum_out + pose_index);
    return ngp_check_launch("frame_ssim");
}
