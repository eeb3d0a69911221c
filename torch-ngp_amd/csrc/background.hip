// Background model of the fused engine (the reference's --bg_radius,
// nerf/network.py:107-129, 202-217 and nerf/renderer.py:272-277): per ray
//   sph = sph_from_ray(o, d, radius)              (k_sph_from_ray's arithmetic)
//   x   = [half(SH4(d)) | hashgrid2D(sph) (4 levels x 2) | 0 (8)]      (32 wide)
//   bg  = sigmoid(W1 . relu(W0 . x))              (FFMLP 32 -> 64 -> 3 of 16)
// in one launch (k_bg_forward), and its backward in two (k_bg_backward,
// k_bg_finish). DESIGN.md section 15.
//
// The MLP runs on v_mfma_f32_16x16x32_f16 in ffmlp.hip's "transposed" form
// (Y^T = W . X^T: the first layer's accumulators are the second layer's B
// operand after the K permutation of ffmlp_pack.h); the A fragments are built
// in LDS with ngp_pack::build_frags from the flat fp16 weights (3072 values:
// no packed image is kept for a network this small).
//
// The backward's sums are order-independent: dW accumulates in fp32 MFMA
// accumulators over each wave's rays (K = ray index, a fixed assignment), and
// every cross-wave sum (the waves' dW tiles, the table scatter) is a 64-bit
// integer atomic add of the contribution in fixed point (2^-24, fp16's
// smallest subnormal) into a scratch. Integer addition is associative, so the
// result does not depend on the atomics' arrival order: a run with the model
// on is bit-reproducible. A contribution that is not finite raises the
// found-inf flag directly; k_bg_finish rounds the scratch to fp16 into the
// gradient buffers, raises the flag for every sum past fp16's range, and
// clears the scratch for the next step.
#include "ffmlp_pack.h"
#include "ngp_common.h"
#include "ngp_step.h"
#include "sh_basis.h"

#include <cmath>

namespace {

using ngp_pack::half8;
using ngp_pack::MatDesc;
using ngp_step::StepState;
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr uint32_t kLevels = 4, kIn = 32, kWidth = 64, kOutPad = 16;
constexpr uint32_t kW0 = kWidth * kIn, kW1 = kOutPad * kWidth, kWeights = kW0 + kW1;
constexpr uint32_t kRays = 64;      // rays per wave step (one per lane)
constexpr uint32_t kGridCol = 16;   // x[16..24): the grid features (after the 16 SH values)
constexpr uint32_t kXLd = 40;       // x tile row pitch in halves (80 B: 16-byte aligned rows)
constexpr uint32_t kHLd = 72;       // hidden tile row pitch in halves (144 B)
constexpr uint32_t kBwdWaves = 4, kBwdThreads = kBwdWaves * kRays;  // backward: one 64-ray step per wave
constexpr uint32_t kMaxBwdBlocks = 64;
constexpr uint32_t kRed = kWidth * kIn + 3 * kWidth;  // dW values that can be nonzero: W0, rows 0..2 of W1
constexpr uint32_t kLvl0Max = 1024;                   // values of grid level 0 a workgroup sums in LDS
constexpr float kRPI = 0.3183098861837907f;
constexpr float kFixed = 16777216.0f, kFixedInv = 1.0f / 16777216.0f;  // 2^24: |v| <= 65504 x 2^29 rays fits
typedef unsigned long long fixed_t;

// sum += v in fixed point; false (nothing added) when v is not finite or past the accumulator's range
NGP_DEV bool add_fixed(fixed_t* p, float v) {  // (p in global memory or in LDS)
    if (!(fabsf(v) < 1.0e12f)) return false;  // (a NaN fails the comparison too); 1e12 x 2^24 < 2^63
    const long long q = __float2ll_rn(v * kFixed);
    if (q != 0) atomicAdd(p, (fixed_t)q);
    return true;
}

struct BgGrid {
    float scale[kLevels];
    uint32_t res[kLevels];
};

// gridencoder.hip make_levels: scale = exp2f(level * S) * H - 1, resolution = ceil(scale) + 1
void make_levels(BgGrid& lv, float S, uint32_t H) {
    for (uint32_t l = 0; l < kLevels; ++l) {
        const float ls = (float)l * S;
        const float e = (float)std::exp2((double)ls);
        const float scale = e * (float)H - 1.0f;
        lv.scale[l] = scale;
        lv.res[l] = (uint32_t)std::ceil(scale) + 1u;
    }
}

NGP_DEV f32x4 mfma(half8 a, half8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }

NGP_DEV MatDesc desc_w0() { return MatDesc{0u, kWidth, kIn, kWidth / 16, 1u, 0u, false}; }
NGP_DEV MatDesc desc_w1() { return MatDesc{kW0, kOutPad, kWidth, 1u, kWidth / 32, kWidth / 16, true}; }
constexpr uint32_t kFrags = kWidth / 16 + kWidth / 32;  // 4 of W0, 2 of W1

// A matrix's NF fragments into LDS by one wave, every load issued before the
// first store (build_frags' load / store pairs cost one memory round trip per
// fragment, a third of these kernels' time at 4096 rays).
template <int NF>
NGP_DEV void load_frags(half8* __restrict__ lds, const ngp_half* __restrict__ w, const MatDesc& m, uint32_t lane) {
    half8 v[NF];
#pragma unroll
    for (int f = 0; f < NF; ++f) v[f] = ngp_pack::frag_slot(w, m, false, (uint32_t)f, lane);
#pragma unroll
    for (int f = 0; f < NF; ++f) lds[(m.frag0 + f) * 64 + lane] = v[f];
}

// the level table's offsets (uniform loads, issued at the kernel's head)
struct LevelOffsets {
    uint32_t v[kLevels + 1];
};
NGP_DEV LevelOffsets load_offsets(const int32_t* __restrict__ offsets) {
    LevelOffsets o;
#pragma unroll
    for (uint32_t l = 0; l <= kLevels; ++l) o.v[l] = (uint32_t)offsets[l];
    return o;
}

// k_sph_from_ray (raymarching.hip), then GridEncoder.forward's (x + 1) / 2
NGP_DEV void sph01(const float* __restrict__ rays_o, const float* __restrict__ rays_d, uint32_t n, float radius,
                   float (&x)[2], float (&d)[3]) {
    const float ox = rays_o[n * 3], oy = rays_o[n * 3 + 1], oz = rays_o[n * 3 + 2];
    const float dx = rays_d[n * 3], dy = rays_d[n * 3 + 1], dz = rays_d[n * 3 + 2];
    const float A = dx * dx + dy * dy + dz * dz;
    const float Bh = ox * dx + oy * dy + oz * dz;
    const float Cc = ox * ox + oy * oy + oz * oz - radius * radius;
    const float t = (-Bh + sqrtf(Bh * Bh - A * Cc)) / A;
    const float px = ox + t * dx, py = oy + t * dy, pz = oz + t * dz;
    const float theta = atan2f(sqrtf(px * px + pz * pz), py);
    const float phi = atan2f(pz, px);
    x[0] = (2 * theta * kRPI - 1 + 1.0f) * 0.5f;
    x[1] = (phi * kRPI + 1.0f) * 0.5f;
    d[0] = dx; d[1] = dy; d[2] = dz;
}

// One level's four corners of k_grid_fwd<D = 2> (hash grid, align_corners
// off, linear): entry indices within the level (always < hs) and weights.
// kExact = false is the forward's arithmetic, bit for bit: the position
// x * scale + 0.5 rounded to fp32 before the cell is taken off, so the
// fraction carries the position's rounding (up to 2^-14 at a scale of 2047).
// kExact = true (the backward's scatter weights) rounds the fraction itself,
// frac = fma(x, scale, 0.5 - cell): within 2^-25 of the real one. The rounded
// position can only reach the next cell's edge from below (an integer is an
// fp32 number), so a negative fraction means the cell before.
struct Corners {
    uint32_t e[4];
    float w[4];
};
template <bool kExact>
NGP_DEV Corners level_corners(const float (&x)[2], float scale, uint32_t res, uint32_t hs) {
    const uint32_t hs_mask = (hs & (hs - 1)) == 0 ? hs - 1 : 0;
    float pos[2];
    uint32_t pg[2];
#pragma unroll
    for (int d = 0; d < 2; ++d) {
        pos[d] = fmaf(x[d], scale, 0.5f);
        pg[d] = (uint32_t)floorf(pos[d]);
        if (kExact) {
            pos[d] = fmaf(x[d], scale, 0.5f - (float)pg[d]);
            if (pos[d] < 0.0f && pg[d] > 0) {
                pg[d] -= 1;
                pos[d] = fmaf(x[d], scale, 0.5f - (float)pg[d]);
            }
        } else {
            pos[d] -= (float)pg[d];
        }
    }
    Corners c;
#pragma unroll
    for (uint32_t idx = 0; idx < 4; ++idx) {
        float w = 1;
        uint32_t pl[2];
#pragma unroll
        for (uint32_t d = 0; d < 2; ++d) {
            if ((idx & (1u << d)) == 0) {
                w *= 1 - pos[d];
                pl[d] = pg[d];
            } else {
                w *= pos[d];
                pl[d] = pg[d] + 1;
            }
        }
        uint32_t stride = 1, index = 0;
#pragma unroll
        for (uint32_t d = 0; d < 2; ++d) {
            if (stride <= hs) {
                index += pl[d] * stride;
                stride *= res + 1;
            }
        }
        if (stride > hs) index = (pl[0] * 1u) ^ (pl[1] * 2654435761u);
        c.e[idx] = hs_mask ? (index & hs_mask) : (index % (hs ? hs : 1u));
        c.w[idx] = w;
    }
    return c;
}

// (F)(half)e of an fp32 table (autocast's embeddings.half() on the fly), or the fp16 copy's value
NGP_DEV float entry_value(float v) { return (float)(ngp_half)v; }
NGP_DEV float entry_value(ngp_half v) { return (float)v; }

// The ray's input row: SH in fp32 rounded to half, the grid features in
// k_grid_fwd<half>'s arithmetic (Acc<half>::mac per corner), 8 zeros.
template <typename E>
NGP_DEV void input_row(const float (&x)[2], const float (&d)[3], const E* __restrict__ table,
                       const LevelOffsets& offsets, const BgGrid& lv, ngp_half (&row)[kIn]) {
    float sh[16];
    ngp_sh::sh_basis<float>(d[0], d[1], d[2], 4u, [&](uint32_t k, float v) { sh[k] = v; });
#pragma unroll
    for (int k = 0; k < 16; ++k) row[k] = ngp_f2h(sh[k]);
    const bool oob = x[0] < 0 || x[0] > 1 || x[1] < 0 || x[1] > 1;
#pragma unroll
    for (uint32_t l = 0; l < kLevels; ++l) {
        ngp_half r0 = (ngp_half)0.0f, r1 = (ngp_half)0.0f;
        if (!oob) {
            const uint32_t off0 = offsets.v[l], hs = offsets.v[l + 1] - off0;
            const Corners c = level_corners<false>(x, lv.scale[l], lv.res[l], hs);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                struct alignas(sizeof(E) * 2) V { E v[2]; };
                const V v = *reinterpret_cast<const V*>(table + ((size_t)off0 + c.e[k]) * 2);
                r0 = Acc<ngp_half>::mac(r0, c.w[k], entry_value(v.v[0]));
                r1 = Acc<ngp_half>::mac(r1, c.w[k], entry_value(v.v[1]));
            }
        }
        row[kGridCol + 2 * l] = r0;
        row[kGridCol + 2 * l + 1] = r1;
    }
#pragma unroll
    for (uint32_t k = kGridCol + 2 * kLevels; k < kIn; ++k) row[k] = (ngp_half)0.0f;
}

NGP_DEV void put_row(ngp_half* dst, const ngp_half (&row)[kIn]) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        half8 v;
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = row[8 * q + j];
        reinterpret_cast<half8*>(dst)[q] = v;
    }
}

// First layer of 16 rays: acc[mt][r] = pre-activation of unit 16 mt + 4 g + r for ray c of the tile
NGP_DEV void layer0(const half8* __restrict__ frags, const ngp_half* __restrict__ xt, uint32_t tile, uint32_t lane,
                    f32x4 (&acc)[4]) {
    const uint32_t g = lane >> 4, c = lane & 15;
    const half8 b = *reinterpret_cast<const half8*>(xt + (16 * tile + c) * kXLd + 8 * g);
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) acc[mt] = mfma(frags[mt * 64 + lane], b, f32x4{0.f, 0.f, 0.f, 0.f});
}

// relu, rounded to half, as the second product's (K-permuted) B operand
NGP_DEV void pack_relu(const f32x4 (&acc)[4], half8 (&hb)[2]) {
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float v = acc[2 * s + (j >> 2)][j & 3];
            hb[s][j] = (ngp_half)(v > 0.0f ? v : 0.0f);
        }
}

// ---- forward ----------------------------------------------------------------
template <typename E>
__global__ void __launch_bounds__(kRays)
k_bg_forward(const float* __restrict__ rays_o, const float* __restrict__ rays_d, float radius, uint32_t N,
             const E* __restrict__ table, const int32_t* __restrict__ offsets, BgGrid lv,
             const ngp_half* __restrict__ weights, float* __restrict__ bg, float* __restrict__ rgba,
             ngp_half* __restrict__ x_save, float* __restrict__ sph_save, float* __restrict__ image,
             const float* __restrict__ weights_sum) {
    __shared__ half8 frags[kFrags * 64];
    __shared__ __attribute__((aligned(16))) ngp_half xt[kRays * kXLd];
    __shared__ float yt[kRays * 4];
    const uint32_t lane = threadIdx.x, n = blockIdx.x * kRays + lane;
    const LevelOffsets lo = load_offsets(offsets);
    load_frags<kWidth / 16>(frags, weights, desc_w0(), lane);
    load_frags<kWidth / 32>(frags, weights, desc_w1(), lane);
    ngp_half row[kIn];
#pragma unroll
    for (uint32_t k = 0; k < kIn; ++k) row[k] = (ngp_half)0.0f;
    if (n < N) {
        float x[2], d[3];
        sph01(rays_o, rays_d, n, radius, x, d);
        input_row(x, d, table, lo, lv, row);
        if (x_save) put_row(x_save + (size_t)n * kIn, row);
        if (sph_save) {
            sph_save[n * 2] = x[0];
            sph_save[n * 2 + 1] = x[1];
        }
    }
    put_row(xt + lane * kXLd, row);
    __syncthreads();
    const uint32_t g = lane >> 4, c = lane & 15;
#pragma unroll
    for (uint32_t t = 0; t < kRays / 16; ++t) {
        f32x4 acc[4];
        layer0(frags, xt, t, lane, acc);
        half8 hb[2];
        pack_relu(acc, hb);
        f32x4 o = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < 2; ++s) o = mfma(frags[(4 + s) * 64 + lane], hb[s], o);
        if (g == 0) {  // outputs 0..3 of ray 16 t + c
#pragma unroll
            for (int r = 0; r < 4; ++r) yt[(16 * t + c) * 4 + r] = o[r];
        }
    }
    __syncthreads();
    if (n >= N) return;
    float y[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        // autocast's half logits and half sigmoid (torch.sigmoid of a half tensor: fp32 inside, rounded)
        const float h = (float)(ngp_half)yt[lane * 4 + k];
        y[k] = (float)(ngp_half)(1.0f / (1.0f + expf(-h)));
        bg[n * 3 + k] = y[k];
    }
    if (rgba) {
        // the white-blended target of a background model (utils.py:508-517), alpha := 1
        const float a = rgba[n * 4 + 3], om = 1 - a;
#pragma unroll
        for (int k = 0; k < 3; ++k) rgba[n * 4 + k] = rgba[n * 4 + k] * a + 1.0f * om;
        rgba[n * 4 + 3] = 1.0f;
    }
    if (image) {
        const float om = 1 - weights_sum[n];
#pragma unroll
        for (int k = 0; k < 3; ++k) image[n * 3 + k] = image[n * 3 + k] + om * y[k];
    }
}

// ---- backward ---------------------------------------------------------------
// Four waves a workgroup, 64 rays per wave step (tiles of its own in LDS) of a
// block-strided loop. scratch: fixed point [table values | kWeights], zero on
// entry (k_bg_finish leaves it so). Atomics to one address serialise, so what
// shares a destination is summed on chip first: the waves' dW tiles in LDS (in
// wave order, fp32), grid level 0 (a few hundred entries that every ray hits)
// in an LDS copy in fixed point; one global atomic per value and workgroup then.
__global__ void __launch_bounds__(kBwdThreads)
k_bg_backward(const int32_t* __restrict__ rays, uint32_t N, const float* __restrict__ out_image,
              const float* __restrict__ out_ws, const float* __restrict__ gt, const float* __restrict__ bg,
              const ngp_half* __restrict__ x_save, const float* __restrict__ sph_save,
              const int32_t* __restrict__ offsets, BgGrid lv, const ngp_half* __restrict__ weights,
              const StepState* __restrict__ st, float color_weight, fixed_t* __restrict__ scratch,
              size_t table_values, int32_t* __restrict__ inf_flag) {
    __shared__ half8 frags[4 * 64];
    __shared__ __attribute__((aligned(16))) ngp_half xt_[kBwdWaves][kRays * kXLd];
    __shared__ __attribute__((aligned(16))) ngp_half ht_[kBwdWaves][kRays * kHLd];  // relu(W0 x)
    __shared__ __attribute__((aligned(16))) ngp_half dt_[kBwdWaves][kRays * kHLd];  // d loss / d (W0 x)
    __shared__ ngp_half gy_[kBwdWaves][kRays * 4];                                  // d loss / d logits (3 of 4)
    __shared__ float w1s[3 * kWidth];                                               // W1 rows 0..2
    __shared__ float w0g[kWidth * 8];                                               // W0[:, 16..24)
    __shared__ fixed_t lvl0[kLvl0Max];
    static_assert(sizeof(ht_) >= kBwdWaves * kRed * sizeof(float), "the dW fold reuses the hidden tiles");
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = lane >> 4, c = lane & 15;
    ngp_half* xt = xt_[wave];
    ngp_half* ht = ht_[wave];
    ngp_half* dt = dt_[wave];
    ngp_half* gy = gy_[wave];
    const LevelOffsets lo = load_offsets(offsets);
    {   // (loads first, then the LDS stores: one round trip): W0's four fragments, one per wave
        const half8 fr = ngp_pack::frag_slot(weights, desc_w0(), false, wave, lane);
        const ngp_half a1 = weights[kW0 + min(tid, 3 * kWidth - 1)];
        ngp_half a0[2];
#pragma unroll
        for (uint32_t q = 0; q < 2; ++q) {
            const uint32_t k = tid + kBwdThreads * q;
            a0[q] = weights[(k >> 3) * kIn + kGridCol + (k & 7)];
        }
        frags[tid] = fr;
        if (tid < 3 * kWidth) w1s[tid] = (float)a1;
#pragma unroll
        for (uint32_t q = 0; q < 2; ++q) w0g[tid + kBwdThreads * q] = (float)a0[q];
        for (uint32_t i = tid; i < kLvl0Max; i += kBwdThreads) lvl0[i] = 0ull;
    }
    const uint32_t n0 = (lo.v[1] - lo.v[0]) * 2;  // level 0's values
    const bool lds0 = n0 <= kLvl0Max;
    // (loss * scale).backward() through mean -> mean(-1) -> pow(2) -> sub, as k_composite_loss
    const float G = ((st->scale * color_weight) * (1.0f / (float)N)) * (1.0f / 3.0f);
    f32x4 dw0[4][2], dw1[4];
    bool bad = false;
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
        dw1[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) dw0[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    for (uint32_t base = blockIdx.x * kBwdThreads; base < N; base += gridDim.x * kBwdThreads) {
        __syncthreads();  // the previous step's tiles are read out (and the prologue's stores are done)
        const uint32_t n = base + tid;
        uint32_t index = n < N ? (rays ? (uint32_t)rays[n * 3] : n) : N;
        const bool valid = index < N;
        if (!valid) index = 0;
        ngp_half gh[4] = {(ngp_half)0.0f, (ngp_half)0.0f, (ngp_half)0.0f, (ngp_half)0.0f};
        half8 xr[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) xr[q] = reinterpret_cast<const half8*>(x_save + (size_t)index * kIn)[q];
        const float x[2] = {sph_save[index * 2], sph_save[index * 2 + 1]};
        if (valid) {
            const float om = 1.0f - out_ws[index];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float e = out_image[index * 3 + k] - gt[index * 4 + k];
                const float y = bg[index * 3 + k];
                const float gb = (G * (2.0f * e)) * om;  // d loss / d bg
                gh[k] = (ngp_half)(gb * (y * (1.0f - y)));
            }
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) xr[q] = half8{0, 0, 0, 0, 0, 0, 0, 0};
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) reinterpret_cast<half8*>(xt + lane * kXLd)[q] = xr[q];
#pragma unroll
        for (int k = 0; k < 4; ++k) gy[lane * 4 + k] = gh[k];
        __syncthreads();
        // the hidden layer again, and its delta = relu'(.) W1^T gy, rounded to half
        // (the loops over tiles and K steps stay rolled: unrolled, the kernel spilled ~200 registers)
#pragma unroll 1
        for (uint32_t t = 0; t < kRays / 16; ++t) {
            f32x4 acc[4];
            layer0(frags, xt, t, lane, acc);
            const uint32_t r0 = 16 * t + c;
            const float g0 = (float)gy[r0 * 4], g1 = (float)gy[r0 * 4 + 1], g2 = (float)gy[r0 * 4 + 2];
#pragma unroll
            for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const uint32_t u = 16 * mt + 4 * g + r;
                    const float v = acc[mt][r];
                    const float d = (w1s[u] * g0 + w1s[kWidth + u] * g1) + w1s[2 * kWidth + u] * g2;
                    ht[r0 * kHLd + u] = (ngp_half)(v > 0.0f ? v : 0.0f);
                    dt[r0 * kHLd + u] = (ngp_half)(v > 0.0f ? d : 0.0f);
                }
        }
        __syncthreads();
        // dW0 += delta^T x, dW1 += gy^T h: M = unit / output, N = input / unit, K = ray
#pragma unroll 1
        for (uint32_t ks = 0; ks < kRays / 32; ++ks) {
            const uint32_t k0 = 32 * ks + 8 * g;
            half8 bx[2], bh[4], ad[4], ag;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) bx[nt][j] = xt[(k0 + j) * kXLd + 16 * nt + c];
#pragma unroll
                for (int mt = 0; mt < 4; ++mt) {
                    bh[mt][j] = ht[(k0 + j) * kHLd + 16 * mt + c];
                    ad[mt][j] = dt[(k0 + j) * kHLd + 16 * mt + c];
                }
                ag[j] = c < 3 ? gy[(k0 + j) * 4 + c] : (ngp_half)0.0f;
            }
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
                dw1[mt] = mfma(ag, bh[mt], dw1[mt]);
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) dw0[mt][nt] = mfma(ad[mt], bx[nt], dw0[mt][nt]);
            }
        }
        // the ray's grid-feature gradient W0[:, 16..24)^T delta, rounded to half
        // (the MLP's fp16 input gradient), scattered with the bilinear weights
        // (level_corners<true>: the fraction rounded once, not the position)
        if (valid) {
            float gi[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll 4
            for (uint32_t u = 0; u < kWidth; ++u) {
                const float d = (float)dt[lane * kHLd + u];
#pragma unroll
                for (int k = 0; k < 8; ++k) gi[k] = fmaf(w0g[u * 8 + k], d, gi[k]);
            }
            const bool oob = x[0] < 0 || x[0] > 1 || x[1] < 0 || x[1] > 1;
            if (!oob) {
#pragma unroll
                for (uint32_t l = 0; l < kLevels; ++l) {
                    const uint32_t off0 = lo.v[l], hs = lo.v[l + 1] - off0;
                    const Corners cn = level_corners<true>(x, lv.scale[l], lv.res[l], hs);
                    const float ga = (float)(ngp_half)gi[2 * l], gb = (float)(ngp_half)gi[2 * l + 1];
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        if (l == 0 && lds0) {  // (e < hs: inside the LDS copy)
                            bad |= !add_fixed(lvl0 + cn.e[k] * 2, cn.w[k] * ga);
                            bad |= !add_fixed(lvl0 + cn.e[k] * 2 + 1, cn.w[k] * gb);
                            continue;
                        }
                        const size_t at = ((size_t)off0 + cn.e[k]) * 2;
                        if (at + 1 < table_values) {
                            bad |= !add_fixed(scratch + at, cn.w[k] * ga);
                            bad |= !add_fixed(scratch + at + 1, cn.w[k] * gb);
                        }
                    }
                }
            }
        }
    }
    // the waves' dW tiles into LDS (over the hidden tiles), summed in wave order
    // accumulator (g, c): rows 4 g + r (M), column c (N)
    __syncthreads();
    float* red = reinterpret_cast<float*>(&ht_[0][0]);
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
                red[wave * kRed + (16 * mt + 4 * g + r) * kIn + 16 * nt + c] = dw0[mt][nt][r];
            if (g == 0 && r < 3) red[wave * kRed + kW0 + r * kWidth + 16 * mt + c] = dw1[mt][r];
        }
    __syncthreads();
    fixed_t* dw = scratch + table_values;  // (rows 0..2 of W1 follow W0 directly, as in red)
    for (uint32_t i = tid; i < kRed; i += kBwdThreads) {
        float sum = red[i];
#pragma unroll
        for (uint32_t w = 1; w < kBwdWaves; ++w) sum += red[w * kRed + i];
        bad |= !add_fixed(dw + i, sum);
    }
    if (lds0) {
        const size_t at0 = (size_t)lo.v[0] * 2;
        for (uint32_t i = tid; i < n0; i += kBwdThreads) {
            const fixed_t v = lvl0[i];
            if (v != 0 && at0 + i < table_values) atomicAdd(scratch + at0 + i, v);
        }
    }
    if (__ballot(bad) && lane == 0) atomicOr(inf_flag, 1);
}

// scratch -> fp16 gradients (4 values per thread), the found-inf flag, scratch := 0
__global__ void __launch_bounds__(256)
k_bg_finish(fixed_t* __restrict__ scratch, size_t table_values, ngp_half* __restrict__ grad_table,
            ngp_half* __restrict__ grad_weights, int32_t* __restrict__ inf_flag) {
    typedef _Float16 half4 __attribute__((ext_vector_type(4)));
    const size_t n4 = (table_values + kWeights) / 4, t4 = table_values / 4;
    bool bad = false;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
        ulonglong2* src = reinterpret_cast<ulonglong2*>(scratch) + 2 * i;
        const ulonglong2 a = src[0], b = src[1];
        half4 h;
        h[0] = ngp_f2h((float)(long long)a.x * kFixedInv);
        h[1] = ngp_f2h((float)(long long)a.y * kFixedInv);
        h[2] = ngp_f2h((float)(long long)b.x * kFixedInv);
        h[3] = ngp_f2h((float)(long long)b.y * kFixedInv);
#pragma unroll
        for (int k = 0; k < 4; ++k) bad |= !__builtin_isfinite((float)h[k]);
        half4* dst = i < t4 ? reinterpret_cast<half4*>(grad_table) + i
                            : reinterpret_cast<half4*>(grad_weights) + (i - t4);
        *dst = h;
        src[0] = src[1] = ulonglong2{0ull, 0ull};
    }
    if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(inf_flag, 1);
}

int check_shapes(const char* who, uint32_t num_levels, uint32_t level_dim, uint32_t input_dim, uint32_t hidden_dim,
                 uint32_t num_layers) {
    NGP_REQUIRE(num_levels == kLevels && level_dim == 2, NGP_ERR_ARG,
                "%s: the background grid has 4 levels of 2 features, got %u x %u", who, num_levels, level_dim);
    NGP_REQUIRE(input_dim == kIn && hidden_dim == kWidth && num_layers == 2, NGP_ERR_UNSUPPORTED,
                "%s: the background MLP is 32 -> 64 -> 3 (2 layers), got input_dim %u hidden_dim %u num_layers %u",
                who, input_dim, hidden_dim, num_layers);
    return NGP_OK;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

extern "C" size_t ngp_background_scratch_bytes(uint64_t table_values) {
    return (size_t)(table_values + kWeights) * sizeof(fixed_t);
}

extern "C" int ngp_background_forward(const float* rays_o, const float* rays_d, float radius, uint32_t N,
                                      const void* table, int32_t table_dtype, const int32_t* offsets,
                                      uint32_t num_levels, uint32_t level_dim, float S, uint32_t H,
                                      const void* weights, uint32_t input_dim, uint32_t hidden_dim,
                                      uint32_t num_layers, float* bg, float* rgba, void* x_save, float* sph_save,
                                      float* image, const float* weights_sum, void* stream) {
    NGP_REQUIRE(rays_o && rays_d && table && offsets && weights && bg, NGP_ERR_ARG,
                "background_forward: null rays, table, offsets, weights or bg");
    NGP_REQUIRE(radius > 0.0f, NGP_ERR_ARG, "background_forward: radius must be > 0, got %g", (double)radius);
    NGP_REQUIRE(N > 0 && N <= 0x7fffffffu / 4u, NGP_ERR_ARG, "background_forward: N must be in [1, 2^29), got %u", N);
    NGP_REQUIRE((image == nullptr) == (weights_sum == nullptr), NGP_ERR_ARG,
                "background_forward: image and weights_sum go together (the inference blend)");
    NGP_REQUIRE(table_dtype == NGP_DTYPE_F32 || table_dtype == NGP_DTYPE_F16, NGP_ERR_ARG,
                "background_forward: the table is fp32 or fp16, got dtype %d", table_dtype);
    if (int e = check_shapes("background_forward", num_levels, level_dim, input_dim, hidden_dim, num_layers)) return e;
    NGP_REQUIRE(aligned16(weights) && aligned16(x_save) && (reinterpret_cast<uintptr_t>(table) & 7u) == 0,
                NGP_ERR_ARG, "background_forward: weights and x_save must be 16-byte aligned, the table 8-byte");
    BgGrid lv;
    make_levels(lv, S, H);
    const dim3 grid(ngp_div_up(N, kRays));
    hipStream_t st = ngp_stream(stream);
    if (table_dtype == NGP_DTYPE_F32)
        k_bg_forward<float><<<grid, kRays, 0, st>>>(rays_o, rays_d, radius, N, static_cast<const float*>(table),
                                                    offsets, lv, static_cast<const ngp_half*>(weights), bg, rgba,
                                                    static_cast<ngp_half*>(x_save), sph_save, image, weights_sum);
    else
        k_bg_forward<ngp_half><<<grid, kRays, 0, st>>>(rays_o, rays_d, radius, N, static_cast<const ngp_half*>(table),
                                                       offsets, lv, static_cast<const ngp_half*>(weights), bg, rgba,
                                                       static_cast<ngp_half*>(x_save), sph_save, image, weights_sum);
    return ngp_check_launch("background_forward");
}

extern "C" int ngp_background_backward(const int32_t* rays, uint32_t N, const float* out_image, const float* out_ws,
                                       const float* gt, const float* bg, const void* x_save, const float* sph_save,
                                       const int32_t* offsets, uint32_t num_levels, uint32_t level_dim, float S,
                                       uint32_t H, uint64_t table_values, const void* weights, uint32_t input_dim,
                                       uint32_t hidden_dim, uint32_t num_layers, const void* state,
                                       float color_weight, float radius, void* scratch, void* grad_table,
                                       void* grad_weights, int32_t* inf_flag, void* stream) {
    NGP_REQUIRE(out_image && out_ws && gt && bg && x_save && sph_save && offsets && weights && state && scratch &&
                    grad_table && grad_weights && inf_flag,
                NGP_ERR_ARG, "background_backward: null buffer");
    NGP_REQUIRE(radius > 0.0f, NGP_ERR_ARG, "background_backward: radius must be > 0, got %g", (double)radius);
    NGP_REQUIRE(N > 0 && N <= 0x7fffffffu / 4u, NGP_ERR_ARG, "background_backward: N must be in [1, 2^29), got %u", N);
    if (int e = check_shapes("background_backward", num_levels, level_dim, input_dim, hidden_dim, num_layers)) return e;
    NGP_REQUIRE(table_values > 0 && table_values % 4 == 0, NGP_ERR_ARG,
                "background_backward: the table's value count must be a positive multiple of 4, got %llu",
                (unsigned long long)table_values);
    NGP_REQUIRE(aligned16(weights) && aligned16(x_save) && aligned16(scratch) &&
                    (reinterpret_cast<uintptr_t>(grad_table) & 7u) == 0 &&
                    (reinterpret_cast<uintptr_t>(grad_weights) & 7u) == 0,
                NGP_ERR_ARG, "background_backward: weights, x_save and scratch must be 16-byte aligned, the "
                             "gradients 8-byte");
    BgGrid lv;
    make_levels(lv, S, H);
    hipStream_t st = ngp_stream(stream);
    const uint32_t blocks = min(ngp_div_up(N, kBwdThreads), kMaxBwdBlocks);
    k_bg_backward<<<blocks, kBwdThreads, 0, st>>>(
        rays, N, out_image, out_ws, gt, bg, static_cast<const ngp_half*>(x_save), sph_save, offsets, lv,
        static_cast<const ngp_half*>(weights), static_cast<const StepState*>(state), color_weight,
        static_cast<fixed_t*>(scratch), (size_t)table_values, inf_flag);
    if (int e = ngp_check_launch("background_backward")) return e;
    const size_t n4 = (size_t)(table_values + kWeights) / 4;
    const uint32_t fblocks = (uint32_t)std::min<size_t>((n4 + 255) / 256, 2048);
    k_bg_finish<<<fblocks, 256, 0, st>>>(static_cast<fixed_t*>(scratch), (size_t)table_values,
                                         static_cast<ngp_half*>(grad_table), static_cast<ngp_half*>(grad_weights),
                                         inf_flag);
    return ngp_check_launch("background_finish");
}
