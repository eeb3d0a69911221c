// The deterministic dW slab reduce of the fused MLP backward (ffmlp.hip
// deferred dW partials, one slab row per backward workgroup), shared by its
// own launch (k_slab_reduce) and the grid backward's bin launch, which can
// carry it as extra blocks (gridencoder.hip): both sum in the same fixed order,
// so the weight gradients are bit-identical either way.
#pragma once
#include "ngp_common.h"


namespace ngp_reduce {

constexpr int kReducePhases = 16;  // row phases of one 64-parameter block
constexpr int kMaxReduceJobs = 4;
constexpr uint32_t kBwdChunkRows = 32;  // rows of one backward chunk (ffmlp.hip: 16 * kNB)
// The slab rows a live-row backward (ngp_nerf_backward_live) writes: its
// workgroup b takes chunks b, b + G, ..., so with nch chunks only rows < nch
// hold partials; rows up to the next multiple of 4 phases are written too
// (zeros), so the reduce's sums keep their association and its result is the
// all-rows sum bit for bit (the rows skipped would add +0.0).
NGP_DEV uint32_t live_slab_rows(int32_t live_count, uint32_t rows) {
    const uint32_t nch = live_count <= 0 ? 0u : ((uint32_t)live_count + kBwdChunkRows - 1) / kBwdChunkRows;
    const uint32_t g = 4u * kReducePhases;
    return min(rows, (nch + g - 1) / g * g);
}
struct ReduceJobs {
    int n;
    const float* slab[kMaxReduceJobs];
    void* out[kMaxReduceJobs];
    uint32_t rows[kMaxReduceJobs], np[kMaxReduceJobs];
    uint32_t block0[kMaxReduceJobs + 1];
    int32_t* nonfinite;  // nullable: set when a written grad is inf/nan (GradScaler's check)
    const int32_t* live;  // nullable: the live-row count of a live-row backward (live_slab_rows)
};

// grad_weights[p] = sum over the slab rows, in a fixed order: row phase ph
// (rows ph, ph + 16, ...) keeps 4 independent partial sums (its loads stay in
// flight), then the 16 phase sums are added in phase order. Block `blk` owns
// 64 parameters; a block of THREADS (64 x 16 or 64 x 8) threads runs 16 /
// (THREADS / 64) phases per thread. part: 16 x 64 floats of LDS.
template <typename OUT, int THREADS>
NGP_DEV void slab_reduce_block(const ReduceJobs& jobs, uint32_t blk, float (*part)[64]) {
    constexpr int WAVES = THREADS / 64, PPT = kReducePhases / WAVES;
    static_assert(kReducePhases % WAVES == 0, "whole phases per thread");
    int j = 0;
    while (j + 1 < jobs.n && blk >= jobs.block0[j + 1]) ++j;
    const float* __restrict__ slab = jobs.slab[j];
    const uint32_t rows = jobs.live ? live_slab_rows(*jobs.live, jobs.rows[j]) : jobs.rows[j], n = jobs.np[j];
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t p = (blk - jobs.block0[j]) * 64 + lane;
#pragma unroll
    for (int q = 0; q < PPT; ++q) {
        const uint32_t ph = wv + (uint32_t)q * WAVES;
        float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
        if (p < n) {
            uint32_t r = ph;
            for (; r + 3 * kReducePhases < rows; r += 4 * kReducePhases) {
                s0 += *(slab + (size_t)r * n + p);
                s1 += *(slab + (size_t)(r + kReducePhases) * n + p);
                s2 += *(slab + (size_t)(r + 2 * kReducePhases) * n + p);
                s3 += *(slab + (size_t)(r + 3 * kReducePhases) * n + p);
            }
            for (; r < rows; r += kReducePhases) s0 += *(slab + (size_t)r * n + p);
        }
        part[ph][lane] = (s0 + s1) + (s2 + s3);
    }
    __syncthreads();
    if (wv == 0 && p < n) {
        float t = 0.0f;
#pragma unroll
        for (int k = 0; k < kReducePhases; ++k) t += part[k][lane];
        const OUT o = (OUT)t;
        static_cast<OUT*>(jobs.out[j])[p] = o;
        if (jobs.nonfinite && !__builtin_isfinite((float)o)) atomicOr(jobs.nonfinite, 1);
    }
}

// ---- the light regime's dW: products from the operand stash -----------------
// With at most rows_max live rows the NeRF backward (ngp_nerf_backward_live_dw,
// ffmlp.hip) forms no dW: per 32-row chunk each wave stashes the operands of
// the dW products instead, transposed ([unit][32 rows] fp16, 64 bytes per
// unit and chunk), so that an MFMA operand of the product below is one
// 16-byte load per lane. A chunk's record is the colour network's arrays, then
// the sigma network's; a network with NH hidden matmuls holds
//   DOUT 16 units at 0      the output gradient (g_color_out / g_h)
//   X    32 units at 16     the input (color_in / enc)
//   H[q] 64 units at 48 + 64 q              post-activations, q = 0..NH
//   D[q] 64 units at 48 + 64 (NH + 1 + q)   deltas of the same layers
// and its weight gradient is dW_0 = D[0]^T X, dW_q = D[q]^T H[q-1] (q = 1..NH),
// dW_last = DOUT^T H[NH], each summed over the live rows. Rows of the last
// chunk past the count are stashed as zeros.
constexpr uint32_t kDwWaves = 8;  // K (the chunks) is split over the waves of a product workgroup
__host__ __device__ constexpr uint32_t dw_net_units(uint32_t nh) { return 48u + 128u * (nh + 1u); }
__host__ __device__ constexpr uint32_t dw_net_tiles(uint32_t nh) { return 8u + 16u * nh + 4u; }  // 16x16 tiles of dW (64 wide, 32 in)
struct DwProduct {
    const void* stash;     // null: no product job, the slab reduce runs whatever the count
    void* out[2];          // fp16 weight gradients: [0] colour, [1] sigma
    uint32_t nh[2];        // hidden matmuls: [0] colour, [1] sigma
    uint32_t B;            // row capacity of the backward (the count is clipped to it)
    uint32_t rows_max;     // light regime: 0 < rows_max and count <= rows_max
    uint32_t blocks;       // product workgroups: one per dW tile of both networks (0: no job)
    uint32_t wgs;          // workgroups of the backward launch (its slab rows)
    const int32_t* live;   // the live-row count
    int32_t* nonfinite;    // nullable: set when a written grad is inf/nan
};
// the live rows of a call (clipped as the backward clips them) and its regime
NGP_DEV uint32_t dw_live_rows(const int32_t* live, uint32_t B) {
    const int32_t n = *live;
    return n <= 0 ? 0u : min(B, (uint32_t)n);
}
NGP_DEV bool dw_light(const DwProduct& dj) {
    return dj.stash && dj.rows_max && dw_live_rows(dj.live, dj.B) <= dj.rows_max;
}

// Workgroup `blk` of kDwWaves waves owns one 16x16 tile of one matmul's dW and
// sums it in the ORDER OF THE SLAB PATH, so the weight gradients are those of
// ngp_nerf_backward_live + the slab reduce bit for bit. The light regime holds
// at most one chunk per backward workgroup (rows_max <= 32 wgs, the host's
// cap), where that path computes, per chunk r, the slab row
//   row[r] = mfma(half 0 of the chunk) + mfma(half 1)     (two waves' 16-row
// half chunks in K slots 0..3 of each lane group, zero accumulators, the fold's
// image0 + image1), and slab_reduce_block then adds the rows per phase
// ph = r % 16 into four partial sums (rows ph, ph + 16, ph + 32, ph + 48 of each
// 64, the remainder into the first), (s0 + s1) + (s2 + s3), and the 16 phase
// sums in phase order. Here wave w runs phases w and w + 8 the same way, with
// row[r] formed from the stash (a record's K slots 8g + 4 half + j are the
// half's slots j) and the rows past the last chunk, zeros there, skipped.
// part: 16 x 256 floats of LDS. No rows: exact zeros.
typedef _Float16 dw_half8 __attribute__((ext_vector_type(8)));
typedef float dw_f32x4 __attribute__((ext_vector_type(4)));
NGP_DEV dw_f32x4 dw_chunk_row(dw_half8 a, dw_half8 b) {
    const dw_f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
    const dw_half8 a0 = {a[0], a[1], a[2], a[3], 0, 0, 0, 0}, a1 = {a[4], a[5], a[6], a[7], 0, 0, 0, 0};
    const dw_half8 b0 = {b[0], b[1], b[2], b[3], 0, 0, 0, 0}, b1 = {b[4], b[5], b[6], b[7], 0, 0, 0, 0};
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a0, b0, z4, 0, 0, 0) +
           __builtin_amdgcn_mfma_f32_16x16x32_f16(a1, b1, z4, 0, 0, 0);
}
NGP_DEV void dw_product_block(const DwProduct& dj, uint32_t blk, float* part) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, c = lane & 15;
    const uint32_t t0 = dw_net_tiles(dj.nh[0]);
    const uint32_t net = blk < t0 ? 0u : 1u, t = blk - net * t0, nh = dj.nh[net];
    // the tile's operands (unit offsets in the chunk record) and its place in the [out][in] weights
    uint32_t au, bu, m, k, in_w, off;
    if (t < 8u) {  // first matmul: D[0]^T X
        m = t >> 1; k = t & 1u; au = 48u + 64u * (nh + 1u); bu = 16u; in_w = 32u; off = 0u;
    } else if (t < 8u + 16u * nh) {  // hidden matmul q: D[q]^T H[q-1]
        const uint32_t q = (t - 8u) / 16u + 1u, l = (t - 8u) % 16u;
        m = l >> 2; k = l & 3u; au = 48u + 64u * (nh + 1u + q); bu = 48u + 64u * (q - 1u); in_w = 64u;
        off = 64u * 32u + (q - 1u) * 64u * 64u;
    } else {  // last matmul: DOUT^T H[NH]
        m = 0u; k = t - 8u - 16u * nh; au = 0u; bu = 48u + 64u * nh; in_w = 64u; off = 64u * 32u + nh * 64u * 64u;
    }
    const uint32_t rec = (dw_net_units(dj.nh[0]) + dw_net_units(dj.nh[1])) * 4u;  // 16-byte words per chunk
    const uint32_t base = net ? dw_net_units(dj.nh[0]) * 4u : 0u;
    const dw_half8* __restrict__ pa = static_cast<const dw_half8*>(dj.stash) + base + (au + 16u * m + c) * 4u + g;
    const dw_half8* __restrict__ pb = static_cast<const dw_half8*>(dj.stash) + base + (bu + 16u * k + c) * 4u + g;
    const uint32_t nch = (dw_live_rows(dj.live, dj.B) + kBwdChunkRows - 1) / kBwdChunkRows;
    const uint32_t R = live_slab_rows((int32_t)dw_live_rows(dj.live, dj.B), dj.wgs);  // the slab rows the reduce adds
    const uint32_t last = min(R, nch);  // rows from here on are zeros
    dw_f32x4* __restrict__ p4 = reinterpret_cast<dw_f32x4*>(part);
#pragma unroll 1
    for (uint32_t h = 0; h < kReducePhases / kDwWaves; ++h) {
        const uint32_t ph = wave + h * kDwWaves;
        dw_f32x4 s[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) s[q] = dw_f32x4{0.f, 0.f, 0.f, 0.f};
        // the reduce's main loop (r + 48 < R): rows r, r + 16, r + 32, r + 48 into s0..s3; then its remainder into s0
        uint32_t r = ph;
        for (; r + 3 * kReducePhases < R; r += 4 * kReducePhases) {  // wave-uniform
            if (r >= last) continue;
            dw_half8 a[4], b[4];
            // unconditional loads (a row past the last chunk reads the last one and is not added)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint32_t cp = min(r + (uint32_t)q * kReducePhases, nch - 1u);
                a[q] = pa[(size_t)cp * rec];
                b[q] = pb[(size_t)cp * rec];
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const dw_f32x4 row = dw_chunk_row(a[q], b[q]);
                if (r + (uint32_t)q * kReducePhases < last) s[q] += row;
            }
        }
        for (; r < last; r += kReducePhases) s[0] += dw_chunk_row(pa[(size_t)r * rec], pb[(size_t)r * rec]);
        p4[ph * 64u + lane] = (s[0] + s[1]) + (s[2] + s[3]);
    }
    __syncthreads();
    if (wave == 0) {
        dw_f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (uint32_t w = 0; w < (uint32_t)kReducePhases; ++w) s += p4[w * 64u + lane];
        // lane (g, c) holds outputs 16m + 4g + r of input 16k + c
        ngp_half* __restrict__ out = static_cast<ngp_half*>(dj.out[net]) + off + (16u * m + 4u * g) * in_w + 16u * k + c;
        bool bad = false;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const ngp_half o = (ngp_half)s[r];
            out[(uint32_t)r * in_w] = o;
            bad |= !__builtin_isfinite((float)o);
        }
        if (dj.nonfinite && bad) atomicOr(dj.nonfinite, 1);
    }
}

// ReduceJobs of n deferred backward calls (ffmlp.hip; the arguments of
// ngp_ffmlp_reduce). Returns the number of 64-parameter blocks (0: nothing).
uint32_t build_reduce_jobs(int32_t n, void* const* workspaces, const uint32_t* Bs, const uint32_t* in_dims,
                           const uint32_t* hidden_dims, const uint32_t* num_layers, void* const* grad_weights,
                           int32_t* nonfinite, ReduceJobs& rj);
// The reduce of built jobs as its own launch (fp16 grads); NGP_OK or an error code.
int launch_slab_reduce(const ReduceJobs& rj, uint32_t blocks, void* stream);
// The product job of the same two networks (ffmlp.hip; [0] sigma, [1] colour);
// NGP_OK or an error code.
int build_dw_product(const uint32_t* Bs, const uint32_t* in_dims, const uint32_t* hidden_dims,
                     const uint32_t* num_layers, void* const* grad_weights, int32_t* nonfinite,
                     const int32_t* live_count, const void* dw_stash, uint32_t dw_stash_rows, uint32_t dw_rows_max,
                     DwProduct& dj);

}  // namespace ngp_reduce
