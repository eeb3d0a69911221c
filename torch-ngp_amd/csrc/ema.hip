// Exponential moving average of a flat fp32 parameter vector: torch_ema's
// ExponentialMovingAverage.update() (the reference trains with ema_decay =
// 0.95, main_nerf.py:219, and updates once per epoch, nerf/utils.py:1051-1052)
//
//   tmp = s - p;  tmp.mul_(1 - decay);  s.sub_(tmp)
//
// in one HBM pass: read s, p; write s (12 B per parameter) where torch makes
// three passes with a temporary (32 B). The three float32 operations keep
// their order and roundings (the library is built with -ffp-contract=off), so
// the shadow equals torch's bit for bit. DESIGN.md §16.
#include "ngp_common.h"

namespace {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kMaxBlocks = 4096;

NGP_DEV float ema(float s, float p, float omd) { return s - omd * (s - p); }

__global__ void __launch_bounds__(kThreads)
k_ema_update(float* __restrict__ shadow, const float* __restrict__ param, uint64_t n, float omd) {
    const uint64_t stride = (uint64_t)gridDim.x * kThreads * 4;
    for (uint64_t i0 = ((uint64_t)blockIdx.x * kThreads + threadIdx.x) * 4; i0 < n; i0 += stride) {
        if (i0 + 4 <= n) {
            float4 s = *reinterpret_cast<const float4*>(shadow + i0);
            const float4 p = *reinterpret_cast<const float4*>(param + i0);
            s.x = ema(s.x, p.x, omd);
            s.y = ema(s.y, p.y, omd);
            s.z = ema(s.z, p.z, omd);
            s.w = ema(s.w, p.w, omd);
            *reinterpret_cast<float4*>(shadow + i0) = s;
        } else {
            for (uint64_t i = i0; i < n; ++i) shadow[i] = ema(shadow[i], param[i], omd);  // the last n % 4
        }
    }
}

}  // namespace

extern "C" int ngp_ema_update(float* shadow, const float* param, uint64_t n, float one_minus_decay, void* stream) {
    if (n == 0) return NGP_OK;
    NGP_REQUIRE(shadow && param, NGP_ERR_ARG, "ema_update: null buffer");
    NGP_REQUIRE(((reinterpret_cast<uintptr_t>(shadow) | reinterpret_cast<uintptr_t>(param)) & 15) == 0, NGP_ERR_ARG,
                "ema_update: shadow and param must be 16-byte aligned");
    uint64_t blocks = ((n + 3) / 4 + kThreads - 1) / kThreads;
    if (blocks > kMaxBlocks) blocks = kMaxBlocks;
    k_ema_update<<<(uint32_t)blocks, kThreads, 0, ngp_stream(stream)>>>(shadow, param, n, one_minus_decay);
    return ngp_check_launch("ema_update");
}
