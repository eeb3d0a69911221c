// Multiresolution hash-grid encoder, forward / backward / TV-grad, for gfx950.
//
// Semantics follow the reference kernels line by line:
//   fast_hash           gridencoder/src/gridencoder.cu:50-63
//   get_grid_index      gridencoder.cu:66-84
//   kernel_grid         gridencoder.cu:87-242   -> k_grid_fwd
//   kernel_grid_backward gridencoder.cu:245-337 -> k_grid_bwd
//   kernel_input_backward gridencoder.cu:340-366 -> k_grid_input_bwd
//   kernel_grad_tv      gridencoder.cu:503-607  -> k_grid_tv
//
// MI355X design:
//   * level-major scheduling: blockIdx.y = level, so the whole chip walks one
//     level's table slice at a time. The largest hashed level is 2^19 entries =
//     2 MiB in fp16, which fits one XCD's 4 MiB L2: the 8 random corner gathers
//     per (point, level) are L2 hits instead of Infinity-Cache hits.
//   * one lane per (point, level) handles all C channels of a corner with one
//     vector access (C=2 fp16: one dword gather, one global_atomic_pk_add_f16).
//   * out_layout 1 writes [B, L*C] directly (what the MLP consumes), removing
//     the reference's permute copy (grid.py:69) and its grad permute (grid.py:87).
//   * per-level scale/resolution are computed once on the host (exp2 in double,
//     rounded to float) and passed as kernel arguments.
//   * a hashed level's size is a power of two: the modulo becomes a mask.
#include "ffmlp_pack.h"
#include "ngp_common.h"
#include "ngp_dpp.h"
#include "ngp_head.h"
#include "ngp_reduce.h"
#include "ngp_step.h"
#include <stdlib.h>

#include <cmath>
#include <type_traits>

namespace {

constexpr uint32_t kMaxLevels = 64;

struct GridLevels {
    float scale[kMaxLevels];
    uint32_t res[kMaxLevels];
};

// reference semantics: scale = exp2f(level * S) * H - 1.0f;
// resolution = (uint32_t)ceil(scale) + 1   (gridencoder.cu:138-139)
static void make_levels(GridLevels& lv, uint32_t L, float S, uint32_t H) {
    for (uint32_t l = 0; l < L; ++l) {
        float ls = (float)l * S;
        float e = (float)std::exp2((double)ls);
        float scale = e * (float)H - 1.0f;
        lv.scale[l] = scale;
        lv.res[l] = (uint32_t)std::ceil(scale) + 1u;
    }
}

template <uint32_t D>
NGP_DEV uint32_t fast_hash(const uint32_t pos_grid[D]) {
    constexpr uint32_t primes[7] = {1u, 2654435761u, 805459861u, 3674653429u,
                                    2097192037u, 1434869437u, 2165219737u};
    uint32_t result = 0;
#pragma unroll
    for (uint32_t i = 0; i < D; ++i) result ^= pos_grid[i] * primes[i];
    return result;
}

// Returns the entry index (not multiplied by C). `hs_mask` is hs-1 when hs is
// a power of two, else 0 (then a true modulo is taken).
template <uint32_t D>
NGP_DEV uint32_t grid_index(uint32_t gridtype, bool align_corners, uint32_t hs, uint32_t hs_mask,
                            uint32_t resolution, const uint32_t pos_grid[D]) {
    uint32_t stride = 1;
    uint32_t index = 0;
#pragma unroll
    for (uint32_t d = 0; d < D && stride <= hs; d++) {
        index += pos_grid[d] * stride;
        stride *= align_corners ? resolution : (resolution + 1);
    }
    if (gridtype == 0 && stride > hs) index = fast_hash<D>(pos_grid);
    return hs_mask ? (index & hs_mask) : (index % hs);
}

NGP_DEV float smoothstep(float v) { return v * v * (3.0f - 2.0f * v); }
NGP_DEV float smoothstep_derivative(float v) { return 6 * v * (1.0f - v); }

// Vector load/store of the C channels of one entry (entries are aligned to
// C*sizeof(T) because offsets are multiples of 8 entries).
template <typename T, uint32_t C>
NGP_DEV void load_entry(const T* __restrict__ p, typename Acc<T>::F out[C]) {
    struct alignas(sizeof(T) * C) V { T v[C]; };
    V x = *reinterpret_cast<const V*>(p);
#pragma unroll
    for (uint32_t c = 0; c < C; ++c) out[c] = (typename Acc<T>::F)x.v[c];
}
// Entry stored as E, computed as T: (F)(T)e, i.e. the reference's
// embeddings.half() applied on the fly to an fp32 table.
template <typename T, typename E, uint32_t C>
NGP_DEV void load_entry_as(const E* __restrict__ p, typename Acc<T>::F out[C]) {
    struct alignas(sizeof(E) * C) V { E v[C]; };
    V x = *reinterpret_cast<const V*>(p);
#pragma unroll
    for (uint32_t c = 0; c < C; ++c) out[c] = (typename Acc<T>::F)(T)x.v[c];
}

// Optional input mapping of the fused train step: x = (raw + shift) * scale
// (GridEncoder.forward's (inputs + bound) / (2 * bound), which torch evaluates
// as a multiply by the fp32 reciprocal), and a device-side row count that
// clips B (rows past the marcher's sample count are not touched).
struct InMap {
    float shift, scale;  // scale == 0: inputs are used as given
    const int32_t* count;
    // backward over a row list (the step's live rows): row b is rows[b], b < *count
    const int32_t* rows = nullptr;
};
NGP_DEV uint32_t phys_row(const InMap& m, uint32_t b) { return m.rows ? (uint32_t)m.rows[b] : b; }
NGP_DEV uint32_t rows_of(uint32_t B, const InMap& m) {
    if (!m.count) return B;
    const int32_t c = *m.count;
    return c <= 0 ? 0u : min(B, (uint32_t)c);
}

template <typename T, uint32_t C>
NGP_DEV void store_entry(T* __restrict__ p, const T in[C]) {
    struct alignas(sizeof(T) * C) V { T v[C]; };
    V x;
#pragma unroll
    for (uint32_t c = 0; c < C; ++c) x.v[c] = in[c];
    *reinterpret_cast<V*>(p) = x;
}

template <typename T, typename E, uint32_t D, uint32_t C>
__global__ void __launch_bounds__(256)
k_grid_fwd(const float* __restrict__ inputs, const E* __restrict__ grid,
           const int32_t* __restrict__ offsets, T* __restrict__ outputs, uint32_t B, uint32_t L,
           GridLevels lv, T* __restrict__ dy_dx, uint32_t gridtype, bool align_corners,
           uint32_t interp, int32_t out_layout, InMap im) {
    using A = Acc<T>;
    using F = typename A::F;
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= rows_of(B, im)) return;
    const uint32_t level = blockIdx.y;

    T* out = out_layout == 0 ? outputs + ((size_t)level * B + b) * C
                             : outputs + ((size_t)b * L + level) * C;

    float x[D];
    bool oob = false;
#pragma unroll
    for (uint32_t d = 0; d < D; d++) {
        x[d] = inputs[(size_t)b * D + d];
        if (im.scale != 0.0f) x[d] = (x[d] + im.shift) * im.scale;
        if (x[d] < 0 || x[d] > 1) oob = true;
    }
    if (oob) {
        T z[C];
#pragma unroll
        for (uint32_t c = 0; c < C; ++c) z[c] = A::zero();
        store_entry<T, C>(out, z);
        if (dy_dx) {
            T* g = dy_dx + (size_t)b * D * L * C + level * D * C;
#pragma unroll
            for (uint32_t i = 0; i < D * C; ++i) g[i] = A::zero();
        }
        return;
    }

    const uint32_t off0 = (uint32_t)offsets[level];
    const uint32_t hs = (uint32_t)offsets[level + 1] - off0;
    const uint32_t hs_mask = (hs & (hs - 1)) == 0 ? hs - 1 : 0;
    const E* __restrict__ g = grid + (size_t)off0 * C;
    const float scale = lv.scale[level];
    const uint32_t resolution = lv.res[level];

    float pos[D], pos_deriv[D];
    uint32_t pg[D];
#pragma unroll
    for (uint32_t d = 0; d < D; d++) {
        pos[d] = fmaf(x[d], scale, align_corners ? 0.0f : 0.5f);
        pg[d] = (uint32_t)floorf(pos[d]);
        pos[d] -= (float)pg[d];
        pos_deriv[d] = 1.0f;  // reference bug at :143 zero-inits d >= 1; see DESIGN.md
        if (interp == 1) {
            pos_deriv[d] = smoothstep_derivative(pos[d]);
            pos[d] = smoothstep(pos[d]);
        }
    }

    typename A::S res[C];
#pragma unroll
    for (uint32_t c = 0; c < C; ++c) res[c] = A::zero();

#pragma unroll
    for (uint32_t idx = 0; idx < (1u << D); idx++) {
        float w = 1;
        uint32_t pl[D];
#pragma unroll
        for (uint32_t d = 0; d < D; d++) {
            if ((idx & (1u << d)) == 0) {
                w *= 1 - pos[d];
                pl[d] = pg[d];
            } else {
                w *= pos[d];
                pl[d] = pg[d] + 1;
            }
        }
        const uint32_t e = grid_index<D>(gridtype, align_corners, hs, hs_mask, resolution, pl);
        F v[C];
        load_entry_as<T, E, C>(g + (size_t)e * C, v);
#pragma unroll
        // (mac_opaque, ngp_common.h: the product is rounded to float, then to half, in every instantiation)
        for (uint32_t c = 0; c < C; ++c) res[c] = A::mac_opaque(res[c], (F)w, v[c]);
    }
    store_entry<T, C>(out, res);

    if (dy_dx) {
        T* dd = dy_dx + (size_t)b * D * L * C + level * D * C;
#pragma unroll
        for (uint32_t gd = 0; gd < D; gd++) {
            typename A::S rg[C];
#pragma unroll
            for (uint32_t c = 0; c < C; ++c) rg[c] = A::zero();
#pragma unroll
            for (uint32_t idx = 0; idx < (1u << (D - 1)); idx++) {
                float w = scale;
                uint32_t pl[D];
#pragma unroll
                for (uint32_t nd = 0; nd < D - 1; nd++) {
                    const uint32_t d = (nd >= gd) ? (nd + 1) : nd;
                    if ((idx & (1u << nd)) == 0) {
                        w *= 1 - pos[d];
                        pl[d] = pg[d];
                    } else {
                        w *= pos[d];
                        pl[d] = pg[d] + 1;
                    }
                }
                pl[gd] = pg[gd];
                const uint32_t il = grid_index<D>(gridtype, align_corners, hs, hs_mask, resolution, pl);
                pl[gd] = pg[gd] + 1;
                const uint32_t ir = grid_index<D>(gridtype, align_corners, hs, hs_mask, resolution, pl);
                F vl[C], vr[C];
                load_entry_as<T, E, C>(g + (size_t)il * C, vl);
                load_entry_as<T, E, C>(g + (size_t)ir * C, vr);
#pragma unroll
                for (uint32_t c = 0; c < C; ++c)
                    rg[c] = A::mac(rg[c], (F)w * (vr[c] - vl[c]), (F)pos_deriv[gd]);
            }
#pragma unroll
            for (uint32_t c = 0; c < C; ++c) dd[gd * C + c] = rg[c];
        }
    }
}

// Forward without dy_dx: two lanes per (point, level). The lane with x bit b
// gathers the 2^(D-1) corners whose x offset is b, which neighbour its
// partner's (x prime 1 / dense stride 1): each gather instruction touches one
// cache line per lane PAIR. The partner's values arrive by one shuffle and
// both lanes accumulate all 2^D corners in the reference's order, so the
// result is bit-identical to k_grid_fwd; the even lane stores it.
//
// XCD-aware block -> work mapping: blocks are dealt round-robin over the 8
// XCDs (MI355X_MICROARCH.md, workgroup dispatch), so block id % 8 picks the
// XCD. XCD j gets only levels j, j + 8, j + 16, ... (each XCD's 4 MiB L2 then
// holds at most ceil(L / 8) level tables), and one block does KL of them for
// its 128 points: the point is loaded once and the KL levels' gathers are all
// in flight together.
//
// Very large batches (B >= kFwdGroupMajorMin, 2^22) run level-group-major with
// one level per block instead: an XCD then works through all points of level
// j before level j + 8, and its L2 holds one level table at a time (two hashed
// fp16 tables are its whole 4 MiB). Same values. The density-grid update's
// 1-2M query points measured faster level-interleaved (r05ad: full update
// 0.655-0.668 -> 0.600-0.609 ms, partial unchanged), hence the threshold.
constexpr uint32_t kFwdLevelsPerBlock = 2;
#ifndef NGP_FWD_LDS
#define NGP_FWD_LDS 0
#endif
constexpr uint32_t kFwdLdsLevels = NGP_FWD_LDS;  // coarse levels served from LDS (k_grid_fwd_lds), 0: none
constexpr uint32_t kFwdLdsMin = 1u << 18;         // points from which they are
constexpr uint32_t kFwdGroupMajorMin = (1u << 22);
// XCD balance of the level-interleaved forward for large batches (the
// density queries; 16 levels: one level pair per XCD): the XCDs whose pair is
// two hashed levels (with a 2^19 table: 5, 6, 7) lend this share of their live
// point chunks to the five XCDs with a dense level. Same values (the same
// per-point work, on another XCD). Same-box A/B (profiles/r06_fwd_borrow_ab.txt):
// density update full 0.576 -> 0.531 ms, partial 0.401 -> 0.374 ms at 15 %
// (25 %: 0.547 / 0.374); the step's ~80K-point forward is not XCD-bound and
// lost 1-2 % with it, hence the threshold.
#ifndef NGP_FWD_BORROW
#define NGP_FWD_BORROW 15
#endif
constexpr uint32_t kFwdBorrowPct = NGP_FWD_BORROW;
constexpr uint32_t kFwdBorrowMin = 1u << 18;  // points (the grid's B) from which the chunks are lent
constexpr uint32_t kFwdBorrowDense = 5;       // the dense levels the host sizes the grid for
__host__ __device__ static inline uint32_t fwd_borrow_pct(uint32_t B) { return B >= kFwdBorrowMin ? kFwdBorrowPct : 0u; }
__host__ __device__ static inline uint32_t fwd_borrow_extra(uint32_t B) {  // blocks per XCD beyond the chunks
    const uint32_t ng = (B + 127) / 128 * fwd_borrow_pct(B) / 100;
    return ((8 - kFwdBorrowDense) * ng + kFwdBorrowDense - 1) / kFwdBorrowDense;
}

// Levels [lo, hi) of the L-level table (the fused step splits the forward
// in two launches, each beside a part of the optimizer sweep); blk is the
// block's index in the forward's part of the grid.
struct LevelRange {
    uint32_t lo, hi;
};

template <typename T, typename E, uint32_t D, uint32_t C, uint32_t KL>
NGP_DEV void grid_fwd_pair_block(uint32_t blk, const float* __restrict__ inputs, const E* __restrict__ grid,
                                 const int32_t* __restrict__ offsets, T* __restrict__ outputs, uint32_t B,
                                 uint32_t L, const GridLevels& lv, uint32_t gridtype, bool align_corners,
                                 uint32_t interp, int32_t out_layout, const InMap& im, LevelRange lr) {
    using A = Acc<T>;
    using F = typename A::F;
    constexpr uint32_t NR = 1u << (D - 1);
    constexpr bool kGroupMajor = KL == 1;
    const uint32_t lpx = (lr.hi - lr.lo + 7) / 8;           // levels per XCD
    const uint32_t gpx = (lpx + KL - 1) / KL;               // level groups per XCD
    const uint32_t k = blk >> 3;
    const uint32_t nch = (B + 127) / 128;                   // point chunks (grid sized on B)
    uint32_t grp = kGroupMajor ? k / nch : k % gpx, chunk = kGroupMajor ? k % nch : k / gpx;
    uint32_t xcd = blk & 7;
    if constexpr (!kGroupMajor && kFwdBorrowPct > 0) {
        if (lr.lo == 0 && lr.hi == 16 && L == 16 && fwd_borrow_pct(B) > 0) {
            // dense levels among 0..7 (a hashed level's table is the finest level's size)
            const uint32_t hmax = (uint32_t)(offsets[16] - offsets[15]);
            uint32_t nd = 0;
#pragma unroll
            for (uint32_t l = 0; l < 8; ++l) nd += (uint32_t)(offsets[l + 1] - offsets[l]) < hmax ? 1u : 0u;
            if (nd == kFwdBorrowDense) {
                const uint32_t live = (rows_of(B, im) + 127) / 128;  // chunks with points
                const uint32_t ng = live * fwd_borrow_pct(B) / 100, nh = 8 - nd;
                grp = 0;
                if (xcd >= nd) {  // a pair of hashed levels: its last ng live chunks are lent
                    chunk = k < live - ng ? k : nch;
                } else if (k < live) {
                    chunk = k;
                } else {  // borrowed: i-th lent chunk, dealt over the dense XCDs
                    const uint32_t i = (k - live) * nd + xcd;
                    chunk = i < nh * ng ? live - ng + i / nh : nch;
                    xcd = i < nh * ng ? nd + i % nh : xcd;
                }
                if (chunk >= nch) return;
            }
        }
    }
    const uint32_t level0 = lr.lo + xcd + 8 * KL * grp;  // this block: level0, level0 + 8, ...
    if (level0 >= lr.hi) return;
    const uint32_t Lfull = L;  // the [B, L, C] layout's row width
    L = lr.hi;                 // the loops below stop at the range's end
    const uint32_t b = chunk * (blockDim.x / 2) + (threadIdx.x >> 1);
    const uint32_t xbit = threadIdx.x & 1;
    const bool live = b < rows_of(B, im);
    if (__ballot(live) == 0) return;  // wave-uniform exit; pairs stay together below

    // Every load below is unconditional (dead lanes read a valid clamped
    // address and discard the value): a load under a divergent branch made the
    // compiler wait vmcnt(0) right after it, so the 2 x 4 gathers of a lane
    // went out one round trip at a time.
    const uint32_t bl = live ? b : 0u;  // some lane of the wave is live, so rows >= 1
    float x[D];
    bool oob = !live;
#pragma unroll
    for (uint32_t d = 0; d < D; d++) {
        const float xi = inputs[(size_t)bl * D + d];
        x[d] = live ? xi : 0.5f;
        if (im.scale != 0.0f) x[d] = (x[d] + im.shift) * im.scale;
        if (x[d] < 0 || x[d] > 1) oob = true;
    }

    // gathers of every level first
    float pos[KL][D];
    F mine[KL][NR][C];
#pragma unroll
    for (uint32_t q = 0; q < KL; ++q) {
        const uint32_t level = level0 + 8 * q;
        if (level >= L) break;
        const uint32_t off0 = (uint32_t)offsets[level];
        const uint32_t hs = (uint32_t)offsets[level + 1] - off0;
        const uint32_t hs_mask = (hs & (hs - 1)) == 0 ? hs - 1 : 0;
        const E* __restrict__ g = grid + (size_t)off0 * C;
        const float scale = lv.scale[level];
        const uint32_t resolution = lv.res[level];
        uint32_t pg[D];
#pragma unroll
        for (uint32_t d = 0; d < D; d++) {
            pos[q][d] = fmaf(x[d], scale, align_corners ? 0.0f : 0.5f);
            pg[d] = (uint32_t)floorf(pos[q][d]);
            pos[q][d] -= (float)pg[d];
            if (interp == 1) pos[q][d] = smoothstep(pos[q][d]);
        }
        // this lane's corners: idx = (rest << 1) | xbit
#pragma unroll
        for (uint32_t rest = 0; rest < NR; rest++) {
            const uint32_t idx = (rest << 1) | xbit;
            uint32_t pl[D];
#pragma unroll
            for (uint32_t d = 0; d < D; d++) pl[d] = (idx & (1u << d)) ? pg[d] + 1 : pg[d];
            // grid_index is < hs for any pl (mask / modulo), so an out-of-bounds
            // point's address is valid too
            const uint32_t e = grid_index<D>(gridtype, align_corners, hs, hs_mask, resolution, pl);
            load_entry_as<T, E, C>(g + (size_t)e * C, mine[q][rest]);
#pragma unroll
            for (uint32_t c = 0; c < C; ++c) mine[q][rest][c] = oob ? (F)0 : mine[q][rest][c];
        }
    }
#pragma unroll
    for (uint32_t q = 0; q < KL; ++q) {
        const uint32_t level = level0 + 8 * q;
        if (level >= L) break;
        typename A::S res[C];
#pragma unroll
        for (uint32_t c = 0; c < C; ++c) res[c] = A::zero();
#pragma unroll
        for (uint32_t idx = 0; idx < (1u << D); idx++) {
            float w = 1;
#pragma unroll
            for (uint32_t d = 0; d < D; d++) w *= (idx & (1u << d)) ? pos[q][d] : 1 - pos[q][d];
            const uint32_t rest = idx >> 1;
#pragma unroll
            for (uint32_t c = 0; c < C; ++c) {
                const F other = (F)ngp_dpp::pair_swap((float)mine[q][rest][c]);  // DPP, every lane active
                const F v = ((idx & 1u) == xbit) ? mine[q][rest][c] : other;
                // (Acc::mac_opaque, ngp_common.h: the D 3, C 2 kernels keep their packed code)
                if constexpr (D == 3 && C == 2) res[c] = A::mac(res[c], (F)w, v);
                else res[c] = A::mac_opaque(res[c], (F)w, v);
            }
        }
        if (live && xbit == 0) {
            if (oob) {
#pragma unroll
                for (uint32_t c = 0; c < C; ++c) res[c] = A::zero();
            }
            T* out = out_layout == 0 ? outputs + ((size_t)level * B + b) * C
                                     : outputs + ((size_t)b * Lfull + level) * C;
            store_entry<T, C>(out, res);
        }
    }
}

template <typename T, typename E, uint32_t D, uint32_t C, uint32_t KL = kFwdLevelsPerBlock>
__global__ void __launch_bounds__(256)
k_grid_fwd_pair(const float* __restrict__ inputs, const E* __restrict__ grid,
                const int32_t* __restrict__ offsets, T* __restrict__ outputs, uint32_t B, uint32_t L,
                GridLevels lv, uint32_t gridtype, bool align_corners, uint32_t interp,
                int32_t out_layout, InMap im, uint32_t lo = 0) {
    grid_fwd_pair_block<T, E, D, C, KL>(blockIdx.x, inputs, grid, offsets, outputs, B, L, lv, gridtype,
                                        align_corners, interp, out_layout, im, LevelRange{lo, L});
}

// north_star's "per-level features staged in LDS" (VERDICT r05 item 2): the
// coarsest dense levels [0, S) of a large batch (the density queries: 1-2M
// points) from a copy of their tables in LDS. Each persistent workgroup reads
// the levels' tables once (fp16 half2 per entry, the value the gathers round
// to: levels 0-1 are 4,920 + 12,168 entries, 67 KB) and then serves every
// corner of its points from LDS instead of the L2 (4 line requests per point
// and level with the lane-pair gathers). Same arithmetic as
// grid_fwd_pair_block (corner order, weights, Acc::mac), so the encodings
// are bit-identical; the pair kernel takes levels [S, L).
template <typename E, uint32_t D, uint32_t S>
__global__ void __launch_bounds__(512)
k_grid_fwd_lds(const float* __restrict__ inputs, const E* __restrict__ grid, const int32_t* __restrict__ offsets,
               ngp_half* __restrict__ outputs, uint32_t B, uint32_t L, GridLevels lv, uint32_t gridtype,
               bool align_corners, uint32_t interp, int32_t out_layout, InMap im) {
    using A = Acc<ngp_half>;
    constexpr uint32_t C = 2;
    extern __shared__ uint32_t tab[];  // half2 bits per entry, levels back to back
    uint32_t lbase[S + 1];
    lbase[0] = 0;
#pragma unroll
    for (uint32_t l = 0; l < S; ++l) {
        const uint32_t off = (uint32_t)offsets[l], hs = (uint32_t)offsets[l + 1] - off;
        for (uint32_t i = threadIdx.x; i < hs; i += blockDim.x) {
            A::F v[C];
            load_entry_as<ngp_half, E, C>(grid + (size_t)(off + i) * C, v);
            const ngp_half2 h{(ngp_half)v[0], (ngp_half)v[1]};
            tab[lbase[l] + i] = __builtin_bit_cast(uint32_t, h);
        }
        lbase[l + 1] = lbase[l] + hs;
    }
    __syncthreads();
    const uint32_t rows = rows_of(B, im);
    for (uint32_t b = blockIdx.x * blockDim.x + threadIdx.x; b < rows; b += gridDim.x * blockDim.x) {
        float x[D];
        bool oob = false;
#pragma unroll
        for (uint32_t d = 0; d < D; d++) {
            x[d] = inputs[(size_t)b * D + d];
            if (im.scale != 0.0f) x[d] = (x[d] + im.shift) * im.scale;
            if (x[d] < 0 || x[d] > 1) oob = true;
        }
#pragma unroll
        for (uint32_t level = 0; level < S; ++level) {
            const uint32_t hs = lbase[level + 1] - lbase[level];
            const uint32_t hs_mask = (hs & (hs - 1)) == 0 ? hs - 1 : 0;
            const float scale = lv.scale[level];
            const uint32_t resolution = lv.res[level];
            float pos[D];
            uint32_t pg[D];
#pragma unroll
            for (uint32_t d = 0; d < D; d++) {
                pos[d] = fmaf(x[d], scale, align_corners ? 0.0f : 0.5f);
                pg[d] = (uint32_t)floorf(pos[d]);
                pos[d] -= (float)pg[d];
                if (interp == 1) pos[d] = smoothstep(pos[d]);
            }
            uint32_t raw[1u << D];
#pragma unroll
            for (uint32_t idx = 0; idx < (1u << D); idx++) {  // every LDS read first
                uint32_t pl[D];
#pragma unroll
                for (uint32_t d = 0; d < D; d++) pl[d] = (idx & (1u << d)) ? pg[d] + 1 : pg[d];
                raw[idx] = tab[lbase[level] + grid_index<D>(gridtype, align_corners, hs, hs_mask, resolution, pl)];
            }
            A::S res[C] = {A::zero(), A::zero()};
#pragma unroll
            for (uint32_t idx = 0; idx < (1u << D); idx++) {
                float w = 1;
#pragma unroll
                for (uint32_t d = 0; d < D; d++) w *= (idx & (1u << d)) ? pos[d] : 1 - pos[d];
                const ngp_half2 h = __builtin_bit_cast(ngp_half2, raw[idx]);
#pragma unroll
                for (uint32_t c = 0; c < C; ++c) res[c] = A::mac(res[c], (A::F)w, oob ? 0.0f : (float)h[c]);
            }
            if (oob) res[0] = res[1] = A::zero();
            ngp_half* out = out_layout == 0 ? outputs + ((size_t)level * B + b) * C : outputs + ((size_t)b * L + level) * C;
            store_entry<ngp_half, C>(out, res);
        }
    }
}

// The fused step's grid forward with the step's tail (ngp_grid_encode_forward_fused_tail):
// the deferred GradScaler / LambdaLR / loss bookkeeping of the update the march
// launch applied (one workgroup, when pending) and the MLP fragment packs from
// the fp16 weights it wrote (one workgroup per pack job), dispatched first,
// beside the forward blocks; the march launch then needs no emit launch after
// it. Neither reads what the forward writes, and the next launch (the MLP
// forward) is the first to read the images or the scale.
struct FwdTail {
    ngp_step::StepState* end;  // null: no bookkeeping block
    ngp_step::ScalerArgs sa;
    const float* loss_ray;
    uint32_t n_rays;
    ngp_pack::PackJobs jobs;
};

template <typename T, typename E, uint32_t D, uint32_t C, uint32_t KL = kFwdLevelsPerBlock>
__global__ void __launch_bounds__(256)
k_grid_fwd_tail(const float* __restrict__ inputs, const E* __restrict__ grid,
                const int32_t* __restrict__ offsets, T* __restrict__ outputs, uint32_t B, uint32_t L,
                GridLevels lv, uint32_t gridtype, bool align_corners, uint32_t interp,
                int32_t out_layout, InMap im, FwdTail ft) {
    uint32_t blk = blockIdx.x;
    if (ft.end) {
        if (blk == 0) {
            if (ft.end->end_pending) ngp_step::step_end_block(ft.end, ft.sa, nullptr, nullptr, ft.loss_ray, ft.n_rays);
            return;
        }
        --blk;
    }
    if (blk < (uint32_t)ft.jobs.n) {
        const ngp_pack::PackJob& j = ft.jobs.job[blk];
        ngp_pack::build_frags(j.image, j.w, j.m, j.transposed != 0);
        return;
    }
    blk -= (uint32_t)ft.jobs.n;
    grid_fwd_pair_block<T, E, D, C, KL>(blk, inputs, grid, offsets, outputs, B, L, lv, gridtype, align_corners,
                                        interp, out_layout, im, LevelRange{0u, L});
}

// ---- scatter-add of one corner's C channels (values already weighted) -----
template <typename T, uint32_t C> struct Scatter;
template <uint32_t C> struct Scatter<float, C> {
    NGP_DEV static void add(float* p, const float v[C]) {
#pragma unroll
        for (uint32_t c = 0; c < C; ++c) atomicAdd(p + c, v[c]);
    }
};
template <uint32_t C> struct Scatter<double, C> {
    NGP_DEV static void add(double* p, const double v[C]) {
#pragma unroll
        for (uint32_t c = 0; c < C; ++c) atomicAdd(p + c, v[c]);
    }
};
template <uint32_t C> struct Scatter<ngp_half, C> {
    NGP_DEV static void add(ngp_half* p, const float v[C]) {
        if constexpr (C % 2 == 0) {
#pragma unroll
            for (uint32_t c = 0; c < C; c += 2) {
                ngp_half2 h = {(ngp_half)v[c], (ngp_half)v[c + 1]};
                __builtin_amdgcn_global_atomic_fadd_v2f16(reinterpret_cast<ngp_half2*>(p + c), h);
            }
        } else {
            // C == 1: packed add of (v, 0) into the aligned dword holding the entry.
            const uintptr_t a = reinterpret_cast<uintptr_t>(p);
            ngp_half2* base = reinterpret_cast<ngp_half2*>(a & ~uintptr_t(3));
            const ngp_half hv = (ngp_half)v[0];
            ngp_half2 h = (a & 2) ? ngp_half2{(ngp_half)0.0f, hv} : ngp_half2{hv, (ngp_half)0.0f};
            __builtin_amdgcn_global_atomic_fadd_v2f16(base, h);
        }
    }
};

// Scatter-add with corner pairing and wave-level merging of identical targets.
//
// Float atomics execute at the memory side, one 64-B request per distinct
// 64-B segment a wave instruction touches (MI355X_MICROARCH.md "Global float
// atomics"), so the request count, not the add count, sets the time. Two
// lanes per (point, level): lane pair (2s, 2s+1) handles the corners with
// x = floor and x = floor + 1 of point s, which are neighbouring entries on
// dense levels and on hashed ones (the x prime of the hash is 1), i.e. one
// request per pair instead of two. Each lane then walks the 2^(D-1) corners
// of the remaining dimensions.
//
// Samples arrive ordered along rays, so on the coarse levels consecutive
// points hit the same cell: per corner, lanes whose target equals that of the
// lane two to the left (same x parity) form a run; a segmented inclusive scan
// (stride-2 shuffles) sums each run into its last lane, which issues ONE
// atomic for the whole run. A ballot skips the scan when nothing collides
// (the fine hashed levels). For fp16 tables each run adds (half)(sum of w*g)
// instead of rounding every term (the reference rounds each term,
// gridencoder.cu:325), i.e. the same values with fewer roundings.
template <typename T, uint32_t D, uint32_t C>
__global__ void __launch_bounds__(256)
k_grid_bwd(const T* __restrict__ grad, const float* __restrict__ inputs,
           const int32_t* __restrict__ offsets, T* __restrict__ grad_grid, uint32_t B, uint32_t L,
           GridLevels lv, uint32_t gridtype, bool align_corners, uint32_t interp,
           int32_t grad_layout, InMap im, uint32_t level0) {
    using A = Acc<T>;
    using F = typename A::F;
    const uint32_t b = blockIdx.x * (blockDim.x / 2) + (threadIdx.x >> 1);
    const uint32_t xbit = threadIdx.x & 1;
    const uint32_t level = level0 + blockIdx.y;
    const int lane = (int)(threadIdx.x & 63);

    bool valid = b < rows_of(B, im);
    const uint32_t pb = valid ? phys_row(im, b) : 0u;  // the sample's row
    float x[D];
#pragma unroll
    for (uint32_t d = 0; d < D; d++) {
        x[d] = valid ? inputs[(size_t)pb * D + d] : 0.5f;
        if (valid && im.scale != 0.0f) x[d] = (x[d] + im.shift) * im.scale;
        if (x[d] < 0 || x[d] > 1) valid = false;  // grad is zero-initialised
    }
    if (__ballot(valid) == 0) return;  // whole wave idle (wave-uniform)

    const uint32_t off0 = (uint32_t)offsets[level];
    const uint32_t hs = (uint32_t)offsets[level + 1] - off0;
    const uint32_t hs_mask = (hs & (hs - 1)) == 0 ? hs - 1 : 0;
    T* __restrict__ gg = grad_grid + (size_t)off0 * C;
    const float scale = lv.scale[level];
    const uint32_t resolution = lv.res[level];

    float pos[D];
    uint32_t pg[D];
#pragma unroll
    for (uint32_t d = 0; d < D; d++) {
        pos[d] = fmaf(x[d], scale, align_corners ? 0.0f : 0.5f);
        pg[d] = (uint32_t)floorf(pos[d]);
        pos[d] -= (float)pg[d];
        if (interp == 1) pos[d] = smoothstep(pos[d]);
    }

    F gcur[C];
    if (valid) {
        const T* gp = grad_layout == 0 ? grad + ((size_t)level * B + pb) * C
                                       : grad + ((size_t)pb * L + level) * C;
        load_entry<T, C>(gp, gcur);
    } else {
#pragma unroll
        for (uint32_t c = 0; c < C; ++c) gcur[c] = 0;
    }

#pragma unroll
    for (uint32_t rest = 0; rest < (1u << (D - 1)); rest++) {
        const uint32_t idx = (rest << 1) | xbit;  // corner bits, dimension 0 = x from the lane
        float w = 1;
        uint32_t pl[D];
#pragma unroll
        for (uint32_t d = 0; d < D; d++) {
            if ((idx & (1u << d)) == 0) {
                w *= 1 - pos[d];
                pl[d] = pg[d];
            } else {
                w *= pos[d];
                pl[d] = pg[d] + 1;
            }
        }
        const uint32_t key = valid ? grid_index<D>(gridtype, align_corners, hs, hs_mask, resolution, pl)
                                   : 0xffffffffu;
        F v[C];
#pragma unroll
        for (uint32_t c = 0; c < C; ++c) v[c] = (F)w * gcur[c];

        const uint32_t kprev = __shfl_up(key, 2, 64);
        const bool same = lane > 1 && kprev == key;
        if (__ballot(same) == 0) {
            if (valid) Scatter<T, C>::add(gg + (size_t)key * C, v);
            continue;
        }
        // run start (same parity) = inclusive max-scan of head positions
        int start = same ? 0 : lane;
#pragma unroll
        for (int o = 2; o < 64; o <<= 1) {
            const int t = __shfl_up(start, o, 64);
            if (lane >= o) start = max(start, t);
        }
#pragma unroll
        for (int o = 2; o < 64; o <<= 1) {
#pragma unroll
            for (uint32_t c = 0; c < C; ++c) {
                const F t = __shfl_up(v[c], o, 64);
                if (lane - o >= start) v[c] += t;
            }
        }
        const uint32_t knext = __shfl_down(key, 2, 64);
        const bool tail = lane >= 62 || knext != key;
        if (valid && tail) Scatter<T, C>::add(gg + (size_t)key * C, v);
    }
}

// ---- binned backward (fused train step) ---------------------------------------
// Scattered atomics cost one memory-side request per (point, corner pair)
// whatever is done, and the coarse levels' few entries turn them into hot
// spots. Instead every level's corner contributions are sorted into bins of
// 2^kBinShift table entries (12, default 2^12 = 4096):
//   k_grid_bwd_bin   one workgroup = kBinPts (512) consecutive samples of one
//                    level; the grid is (level, block), levels interleaved.
//                    Consecutive samples walk along a ray, so on coarse
//                    levels neighbouring lanes sit in one cell: runs of
//                    samples in one cell are summed in-wave (one segmented DPP
//                    scan carrying all corners) and only the run's last lane
//                    keeps the items. Items are ranked per bin in LDS (few-bin
//                    levels: one LDS atomic instruction for up to 8 bins of
//                    the wave), each bin's run is reserved with one global
//                    atomic and written contiguously.
//   k_grid_bin_accum persistent; a work unit = up to kSegItems items of one
//                    bin, summed exactly in an LDS image of int64 fixed-point
//                    counts of the bin's entries. A unit that owns its bin
//                    stores the slice (per entry, or per item for small units
//                    of a cleared grad); the units of a bin with several add
//                    their images into the bin's int64 slot and the last to
//                    arrive stores the slice.
// Contributions are rounded to half once per run (the reference rounds each
// term, gridencoder.cu:325) and summed exactly. Items past a bin's capacity
// (a concentrated sample cloud) are added as the same int64 counts into a
// spill image of the table with integer atomics, and the bin's first unit
// folds its slice of the spill image into its own before storing: every sum
// is exact and independent of arrival order in every regime, so the result
// is one fp16 rounding of the exact sum of the rounded runs, bit-identical
// from launch to launch. Levels with more than kMaxBinsPerLevelBig bins (or
// past the plan's kMaxTotalBins) use k_grid_bwd.
// The NGP_* macros exist only for same-box A/B builds (tools/variants.sh).
constexpr uint32_t kBinShift = 12;
constexpr uint32_t kBinEntries = 1u << kBinShift;
constexpr uint32_t kMaxBinsPerLevel = 256;       // the bin kernel's small instantiation
constexpr uint32_t kMaxBinsPerLevelBig = 1024;   // ... and the large one (2^22-entry levels)
// the accumulate keeps two words per bin in LDS beside its 64 KiB image
constexpr uint32_t kMaxTotalBins = 11776;
constexpr uint32_t kSegItems = 16384;
// entries within a bin are packed in 16 bits while staged (| bin << 16)
static_assert(kBinShift >= 9 && kBinShift <= 16, "12 must be in [9, 16]");
static_assert(kSegItems > 0, "16384 must be positive");
// Levels up to this resolution merge runs of equal corners in-wave: on the
// Lego step the merge cuts their items 3.5-16x (tools/grid_bwd_micro.py);
// finer levels gain less than the scan costs. Round 7: 128 -> 256. The live
// rows are runs of consecutive samples at the surface, which share corners up
// to res ~300: unmerged, levels 7-8's bins held ~4 items per distinct entry
// (per-wave stamps, r07h); same box +3.5 % (r07i: m256 vs base).
#ifndef NGP_MERGE_MAX_RES
#define NGP_MERGE_MAX_RES 256
#endif
constexpr uint32_t kMergeMaxRes = NGP_MERGE_MAX_RES;

struct BinPlan {
    uint32_t nlev;                   // levels [0, nlev) are binned
    uint32_t total_bins;
    uint64_t merge_mask;             // levels whose equal-corner runs are merged in-wave (one bit per level, kMaxLevels <= 64)
    uint32_t nbins[kMaxLevels];
    uint32_t bin0[kMaxLevels];       // first global bin of the level
    uint32_t cap[kMaxLevels];        // item capacity per bin
    uint32_t item0[kMaxLevels];      // first item slot of the level; bin b at item0 + b * cap
    // bins that may hold more than one work unit (cap > kSegItems: the dense
    // levels) get a slot of int64 sums + an arrival counter: the units add
    // their exact partial sums there and the last one to arrive finishes the
    // bin, so its result does not depend on the units' order
    uint32_t mslot0[kMaxLevels];     // first slot of the level's bins, or kNoSlot
    uint32_t nmslots;
    uint32_t spill_entries;          // table entries of the binned levels (the spill image's size)
    uint32_t img_bins;               // bins of the leading dense levels (z-slab bins); the rest are hashed
    uint32_t off[kMaxLevels + 1];    // the levels' first table entries (offsets), levels [0, nlev]
};
constexpr uint32_t kNoSlot = 0xffffffffu;

struct BinItem {  // 8 bytes: the accumulate kernel reads items as one dword pair
    uint32_t e;                      // entry within the bin (| bin << 16 while staged)
    ngp_half2 v;
};
static_assert(sizeof(BinItem) == 8, "BinItem layout");

// An fp16 value as a signed count of 2^-24 (every finite fp16 is one:
// (1024 + m) << (e - 1) for normals, m for subnormals); |x| < 2^41.
NGP_DEV int64_t half_fixed24(uint32_t bits) {
    const uint32_t e = (bits >> 10) & 31u, m = bits & 1023u;
    const int64_t mag = e ? (int64_t)(1024u | m) << (e - 1) : (int64_t)m;
    return (bits & 0x8000u) ? -mag : mag;
}

NGP_DEV uint32_t lanes_below(uint64_t m) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

#ifndef NGP_BIN_PTS
#define NGP_BIN_PTS 512
#endif
constexpr uint32_t kBinPts = NGP_BIN_PTS;  // samples (threads) per bin-kernel workgroup
#ifndef NGP_BIN_WAVES
#define NGP_BIN_WAVES 6
#endif
constexpr uint32_t kBinWavesPerSimd = NGP_BIN_WAVES;  // the bin kernel's occupancy bound (8: <= 64 VGPRs, spills)
#ifndef NGP_SPLIT_BITS
#define NGP_SPLIT_BITS 6
#endif
constexpr uint32_t kSplitBits = NGP_SPLIT_BITS;  // levels of <= 2^kSplitBits bins rank by wave multisplit
static_assert(kBinPts % 64 == 0 && kBinPts >= 128 && kBinPts <= 1024, "whole waves, 2..16 per workgroup");
#ifndef NGP_BIN_YCAP
#define NGP_BIN_YCAP 0xffffffffu
#endif
constexpr uint32_t kBinYCap = NGP_BIN_YCAP;  // point blocks per level in the grid (each workgroup loops)
// NGP_GRID_TIMING ring (u32 words): [0] calls, heads {start, samples,
// accumulate workgroups, -} from word 64, per-workgroup ends from kTimingEnds
constexpr uint32_t kTimingHeads = 64, kTimingEnds = kTimingHeads + 4 * NGP_GRID_TIMING_RING;

// Workgroup barrier that orders LDS only: unlike __syncthreads() it does not
// wait for the wave's outstanding global loads, stores and atomics.
NGP_DEV void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// Loads of bytes another workgroup of the SAME launch stored (the one-launch
// grid backward, k_grid_bwd_fused): `sc1` loads, L2-served, never a stale L1
// line; the producer stores those bytes `sc1` too and signals after its waves'
// vmcnt(0) waits and a workgroup barrier (MI355X_MICROARCH.md, inter-workgroup
// visibility: the first hand-off row). Two launches need neither.
template <bool SC1> NGP_DEV uint64_t ld_u64(const uint64_t* p) {
    if constexpr (SC1) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else return __builtin_nontemporal_load(p);
}
template <bool SC1> NGP_DEV uint32_t ld_u32(const uint32_t* p) {
    if constexpr (SC1) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else return *p;
}
template <bool SC1> NGP_DEV ulonglong2 ld_u64x2(const unsigned long long* p) {
    if constexpr (SC1) return ulonglong2{ld_u64<true>(reinterpret_cast<const uint64_t*>(p)),
                                         ld_u64<true>(reinterpret_cast<const uint64_t*>(p) + 1)};
    else return *reinterpret_cast<const ulonglong2*>(p);
}

#ifdef NGP_STAMPS  // diagnostic build only (tools/accum_stamps.py): per-workgroup phase clocks
__device__ unsigned long long* g_stamps;
#define STAMP(slot, v) do { if (g_stamps && threadIdx.x == 0) g_stamps[blockIdx.x * 64 + (slot)] = (v); } while (0)
#define BSTAMP(slot) do { if (g_stamps && threadIdx.x == 0) g_stamps[32768 + (size_t)stamp_id * 16 + (slot)] = __builtin_amdgcn_s_memtime(); } while (0)
// the chip-wide 100 MHz clock (s_memtime counts per shader engine / CU and
// cannot order workgroups against each other)
#define BRSTAMP(slot) do { if (g_stamps && threadIdx.x == 0) g_stamps[32768 + (size_t)stamp_id * 16 + (slot)] = __builtin_amdgcn_s_memrealtime(); } while (0)
#define RSTAMP(slot) STAMP(slot, __builtin_amdgcn_s_memrealtime())
// per wave (lane 0) of the accumulate's wave bins: [n | level << 32 | spilled << 40, start, end]
#define WSTAMP(slot, v) do { if (g_stamps && (threadIdx.x & 63) == 0) g_stamps[131072 + (size_t)(blockIdx.x * (kAccThreads / 64) + (threadIdx.x >> 6)) * 4 + (slot)] = (v); } while (0)
// after the wave's outstanding loads have arrived
#define BSTAMPW(slot) do { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); BSTAMP(slot); } while (0)
#define XSTAMP(role, by, k) do { if (g_stamps && threadIdx.x == 0 && (by) < 4096) g_stamps[200000 + ((size_t)(role) * 4096 + (by)) * 2 + (k)] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define BSTAMPW(slot) do { } while (0)
#define WSTAMP(slot, v) do { } while (0)
#define XSTAMP(role, by, k) do { } while (0)
#define BRSTAMP(slot) do { } while (0)
#define RSTAMP(slot) do { } while (0)
#define STAMP(slot, v) do { } while (0)
#define BSTAMP(slot) do { } while (0)
#endif

// The next batch of the fused step drawn as one more column of the bin
// launch (ngp_grid_encode_backward_fused_reduce_batch): nlego blocks of the
// sampler (ngp_head::lego_rays_block), counter kept (the accumulate resets it)
struct BinLego {
    ngp_head::LegoScene sc;
    ngp_head::LegoOut out;
    const float* poses;
    ngp_step::StepState* st;
    uint32_t N, nlego;
};

// The bin launch's LDS, carved from one region (the one-launch form reuses
// the accumulate's image for it): counters, scan offsets, per-bin staging
// info, then the staged items.
template <uint32_t NBMAX> constexpr size_t bin_lds_words() {
    return (2 * (size_t)NBMAX + 1 + kBinPts / 64 + 1 + 1) / 2 * 2 + 2 * (size_t)NBMAX + 2 + (size_t)kBinPts * 8 * 2;
}

template <uint32_t D, uint32_t NBMAX, bool SC1>
NGP_DEV void bin_block(const ngp_half* __restrict__ grad, const float* __restrict__ inputs,
                       const int32_t* __restrict__ offsets, ngp_half* __restrict__ grad_grid, uint32_t B,
                       uint32_t L, const GridLevels& lv, uint32_t gridtype, bool align_corners, uint32_t interp,
                       const InMap& im, const BinPlan& bp, uint32_t* __restrict__ cursor, BinItem* __restrict__ items,
                       int32_t grad_layout, int32_t* __restrict__ nonfinite, const ngp_reduce::ReduceJobs& rj,
                       uint32_t nred, uint32_t* __restrict__ timing, const BinLego& next_batch,
                       unsigned long long* __restrict__ spill, uint32_t* __restrict__ spill_bad,
                       uint32_t* __restrict__ rows_out, uint32_t bx, uint32_t by, uint32_t gy, uint32_t* lds,
                       const ngp_reduce::DwProduct& dw) {
    constexpr uint32_t NC = 1u << D, NW = kBinPts / 64;
    constexpr uint32_t BPT = (NBMAX + kBinPts - 1) / kBinPts;  // bins per thread in the reservation step
    uint32_t* cnt = lds;                 // [NBMAX]
    uint32_t* soff = cnt + NBMAX;        // [NBMAX + 1]
    uint32_t* wsum = soff + NBMAX + 1;   // [NW]
    uint32_t& s_over = wsum[NW];         // some bin of this workgroup ran past its capacity
    uint2* binfo = reinterpret_cast<uint2*>(lds + (2 * NBMAX + 1 + NW + 1 + 1) / 2 * 2);  // (slot - stage index, end of the bin's in-capacity stage run)
    BinItem* stage = reinterpret_cast<BinItem*>(binfo + NBMAX + 1);  // kBinPts * NC
    // launch timing (NGP_GRID_TIMING): block (0, 0), dispatched first, opens
    // this call's ring entry: start on the chip's constant 100 MHz clock, the
    // samples, the call count (plain stores: one thread, and the previous
    // call's kernels have finished)
    // the rows this call bins, for the accumulate's regime choice
    if (rows_out && (bx | by) == 0 && threadIdx.x == 0) *rows_out = rows_of(B, im);
    if (timing && (bx | by) == 0 && threadIdx.x == 0) {
        const uint32_t c = timing[0];
        uint32_t* h = timing + kTimingHeads + (c % NGP_GRID_TIMING_RING) * 4;
        h[0] = (uint32_t)__builtin_amdgcn_s_memrealtime();
        h[1] = rows_of(B, im);
        if constexpr (SC1)  // read by the same launch's accumulate workgroups
            __hip_atomic_store(timing, c + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else
            timing[0] = c + 1;
    }
    // the extra column of blocks (x == nlev): the MLP dW slab reduce, which
    // neither needs nor feeds this kernel (one launch less per step; the same
    // fixed summation order as k_slab_reduce, ngp_reduce.h)
    // and the column after it (x == nlev + (nred != 0)): the next batch's
    // sampler blocks, when the launch carries it
    if (bx >= bp.nlev) {
        // (stamps build: each extra block's start / end on the constant clock,
        // role 0 the dW reduce, role 1 the sampler)
        // When the launch carries a dW product job (ngp_reduce.h), the reduce
        // column is the product column in the light regime of
        // ngp_nerf_backward_live_dw: its first dw.blocks workgroups (one per
        // dW tile, never more than the reduce's blocks) form the weight
        // gradients from the stash and the others return at once; in the
        // other regime the column is the slab reduce as ever, so that launch
        // has the same workgroups as one without the job.
        [[maybe_unused]] const uint32_t xrole = nred && bx == bp.nlev ? 0u : 1u;
        XSTAMP(xrole, by, 0);
        if (nred && bx == bp.nlev) {
            if (ngp_reduce::dw_light(dw)) {
                if (by < dw.blocks) ngp_reduce::dw_product_block(dw, by, reinterpret_cast<float*>(stage));
            } else if (by < nred) {
                ngp_reduce::slab_reduce_block<ngp_half, kBinPts>(rj, by, reinterpret_cast<float(*)[64]>(stage));
            }
        } else if (by < next_batch.nlego) {
            const BinLego& q = next_batch;
            ngp_head::lego_rays_block(by, q.nlego, q.poses, q.sc, q.N, q.st, q.out);
        }
        XSTAMP(xrole, by, 1);
        return;
    }
    // the grid covers the row capacity; workgroups past the marched sample
    // count (about a fifth of them on the Lego step) leave before any work
    // grid (level, point block): consecutive workgroups take different levels
    // of one block, so the coarse levels' VALU-heavy merging (dispatched
    // first and alone when the grid was level-major: 9-16 us per workgroup
    // against 6-8 us on the fine levels) shares the CUs with the fine levels'
    // latency-bound work
    // A workgroup takes point blocks blockIdx.y, blockIdx.y + gridDim.y, ...:
    // the host may cap the grid's height below the row capacity (most of a
    // capacity-sized grid exits at once in the live-row regime)
    const uint32_t level = bx;
    const uint32_t rows = rows_of(B, im);
    for (uint32_t chunk = by; chunk * kBinPts < rows; chunk += gy) {
    if (chunk != by) __syncthreads();  // the last block's write-out has read the LDS
    [[maybe_unused]] const uint32_t stamp_id = level * gy + chunk;
    const uint32_t nb = bp.nbins[level];
    const bool merge = (bp.merge_mask >> level) & 1ull;
    const int lane = (int)(threadIdx.x & 63);
    for (uint32_t j = threadIdx.x; j < nb; j += kBinPts) cnt[j] = 0;
    lds_barrier();
    BSTAMP(0);
    BRSTAMP(8);

    const uint32_t b = chunk * kBinPts + threadIdx.x;
    const bool in_rows = b < rows;
    // the sample's coordinates and this level's grad are loaded together (the
    // grad of an out-of-bounds sample is discarded below): loads gated on the
    // previous coordinate's bounds check went out one round trip at a time
    const uint32_t bl = in_rows ? phys_row(im, b) : 0u;  // the sample's row
    float x[D];
#pragma unroll
    for (uint32_t d = 0; d < D; d++) x[d] = inputs[(size_t)bl * D + d];
    const size_t gi0 = grad_layout == 0 ? (size_t)level * B + bl : (size_t)bl * L + level;
    const ngp_half2 gv0 = *reinterpret_cast<const ngp_half2*>(grad + gi0 * 2);
    bool valid = in_rows;
#pragma unroll
    for (uint32_t d = 0; d < D; d++) {
        if (!in_rows) x[d] = 0.5f;
        if (in_rows && im.scale != 0.0f) x[d] = (x[d] + im.shift) * im.scale;
        if (x[d] < 0 || x[d] > 1) valid = false;
    }
    const uint32_t off0 = (uint32_t)offsets[level];
    const uint32_t hs = (uint32_t)offsets[level + 1] - off0;
    const uint32_t hs_mask = (hs & (hs - 1)) == 0 ? hs - 1 : 0;
    const float scale = lv.scale[level];
    const uint32_t resolution = lv.res[level];
    float pos[D];
    uint32_t pg[D];
#pragma unroll
    for (uint32_t d = 0; d < D; d++) {
        pos[d] = fmaf(x[d], scale, align_corners ? 0.0f : 0.5f);
        pg[d] = (uint32_t)floorf(pos[d]);
        pos[d] -= (float)pg[d];
        if (interp == 1) pos[d] = smoothstep(pos[d]);
    }
    const float g0 = valid ? (float)gv0[0] : 0.0f, g1 = valid ? (float)gv0[1] : 0.0f;
    if (g0 == 0.0f && g1 == 0.0f) valid = false;  // nothing to add (e.g. samples past the early stop)
    BSTAMPW(5);

    uint32_t key[NC], rank[NC];
    ngp_half2 val[NC];
    bool live[NC];
    float vv[NC][2];
#pragma unroll
    for (uint32_t idx = 0; idx < NC; idx++) {
        float w = 1;
        uint32_t pl[D];
#pragma unroll
        for (uint32_t d = 0; d < D; d++) {
            if ((idx & (1u << d)) == 0) {
                w *= 1 - pos[d];
                pl[d] = pg[d];
            } else {
                w *= pos[d];
                pl[d] = pg[d] + 1;
            }
        }
        const uint32_t k = valid ? grid_index<D>(gridtype, align_corners, hs, hs_mask, resolution, pl)
                                 : 0xffffffffu;
        key[idx] = k;
        live[idx] = valid;
        vv[idx][0] = w * g0;
        vv[idx][1] = w * g1;
    }
    if (merge) {
        // Consecutive samples in one cell share all 2^D corners: one run
        // structure (cell equality with the previous lane) and one segmented
        // DPP scan carrying every corner's pair, the run's last lane keeping
        // the sums. Per corner (a key compare, a ballot and a scan each) this
        // was the coarse levels' VALU bottleneck.
        // (every lane moves its values: a DPP move reading a lane that is off
        // in EXEC -- as under a short-circuited condition -- yields 0)
        const uint32_t vprev = ngp_dpp::prev_lane(valid ? 1u : 0u);
        uint32_t pprev[D];
#pragma unroll
        for (uint32_t d = 0; d < D; d++) pprev[d] = ngp_dpp::prev_lane(pg[d]);
        bool same = valid && lane > 0 && vprev != 0;
#pragma unroll
        for (uint32_t d = 0; d < D; d++) same = same && pprev[d] == pg[d];
        const uint64_t sm = __ballot(same);
        if (sm) {
            ngp_dpp::seg_scan_pairs<NC>(vv, !same);
            const bool next_same = lane < 63 && ((sm >> (lane + 1)) & 1ull);
#pragma unroll
            for (uint32_t idx = 0; idx < NC; idx++) live[idx] = valid && !next_same;
        }
    }
#pragma unroll
    for (uint32_t idx = 0; idx < NC; idx++) val[idx] = ngp_half2{(ngp_half)vv[idx][0], (ngp_half)vv[idx][1]};
    // Rank within the bin (the item's slot in the workgroup's run of its bin).
    // On levels of at most 2^kSplitBits bins (round 7) the ranks come from a
    // wave multisplit: per corner, the lanes whose items share my bin
    // are found with one ballot per bin bit (no LDS), the lowest of them
    // reserves the group's run with one LDS atomic (one instruction for all
    // of the wave's groups, distinct addresses) and a lane permute hands the
    // base to the others. The match loop this replaced (up to 8 rounds of 8
    // ballots and read-lanes, then per-item atomics on the few counters every
    // lane hits) was the bin launch's critical path in the live-row regime:
    // 12-16 K cycles on the dense levels against ~3-4 K elsewhere (phase
    // clocks, r07c). Other levels: one LDS atomic per wave when the corner's
    // items share one bin, else one per item.
    BSTAMP(6);
    const uint32_t nbits = nb > 1 ? 32u - (uint32_t)__builtin_clz(nb - 1u) : 0u;
#pragma unroll
    for (uint32_t idx = 0; idx < NC; idx++) rank[idx] = 0;
    if (nbits <= kSplitBits) {
#pragma unroll
        for (uint32_t idx = 0; idx < NC; idx++) {
            const uint32_t bin = key[idx] >> kBinShift;  // garbage for a dead item: it is not in any ballot
            uint64_t m = __ballot(live[idx]);
            for (uint32_t bt = 0; bt < nbits; ++bt) {
                const bool bit = ((bin >> bt) & 1u) != 0;
                const uint64_t bb = __ballot(live[idx] && bit);
                m &= bit ? bb : ~bb;
            }
            // m (live lanes): the lanes whose item of this corner is in my bin
            const int leader = m ? __ffsll((unsigned long long)m) - 1 : lane;
            uint32_t base = 0;
            if (live[idx] && lane == leader) base = atomicAdd(&cnt[bin], (uint32_t)__popcll(m));
            base = (uint32_t)__shfl((int)base, leader, 64);
            if (live[idx]) rank[idx] = base + lanes_below(m);
        }
    } else {
#pragma unroll
        for (uint32_t idx = 0; idx < NC; idx++) {
            const uint64_t lm = __ballot(live[idx]);
            if (!lm) continue;
            const bool mine = (lm >> lane) & 1ull;
            const uint32_t bin = key[idx] >> kBinShift;
            const int first = __ffsll((unsigned long long)lm) - 1;
            const uint32_t bf = __builtin_amdgcn_readlane(bin, first);
            if (__ballot(mine && bin != bf) == 0) {
                uint32_t r0 = 0;
                if (lane == first) r0 = atomicAdd(&cnt[bf], (uint32_t)__popcll(lm));
                if (mine) rank[idx] = __builtin_amdgcn_readlane(r0, first) + lanes_below(lm);
            } else if (mine) {
                rank[idx] = atomicAdd(&cnt[bin], 1u);
            }
        }
    }
    lds_barrier();
    BSTAMP(1);
    // reserve each bin's run now (one global atomic per bin); the results are
    // needed only by the write-out, so the scan and the staging overlap them.
    // The part of a run past the bin's capacity goes atomic, so slots
    // [0, min(cursor, cap)) are always all written.
    const uint32_t cap = bp.cap[level];
    // thread t owns bins t*BPT .. t*BPT + BPT - 1 (contiguous, in scan order)
    uint32_t c_mine[BPT], bs_mine[BPT], c_sum = 0;
#pragma unroll
    for (uint32_t j = 0; j < BPT; ++j) {
        const uint32_t bj = threadIdx.x * BPT + j;
        c_mine[j] = bj < nb ? cnt[bj] : 0u;
        bs_mine[j] = 0;
        if (c_mine[j]) bs_mine[j] = atomicAdd(&cursor[bp.bin0[level] + bj], c_mine[j]);
        c_sum += c_mine[j];
    }
    {   // block-wide exclusive scan of cnt[0..nb)
        const uint32_t t = threadIdx.x, wv = t >> 6;
        const uint32_t incl = ngp_dpp::scan_incl_u32(c_sum);
        if (lane == 63) wsum[wv] = incl;
        lds_barrier();
        uint32_t before = 0, all = 0;
#pragma unroll
        for (uint32_t w = 0; w < NW; ++w) {
            before += w < wv ? wsum[w] : 0u;
            all += wsum[w];
        }
        uint32_t run = before + incl - c_sum;
#pragma unroll
        for (uint32_t j = 0; j < BPT; ++j) {
            const uint32_t bj = t * BPT + j;
            if (bj < nb) soff[bj] = run;
            run += c_mine[j];
        }
        if (t == 0) soff[nb] = all;
    }
    lds_barrier();
    BSTAMP(2);
#pragma unroll
    for (uint32_t idx = 0; idx < NC; idx++) {
        if (!live[idx]) continue;
        const uint32_t bin = key[idx] >> kBinShift;
        stage[soff[bin] + rank[idx]] = BinItem{(key[idx] & (kBinEntries - 1)) | (bin << 16), val[idx]};
    }
    if (threadIdx.x == 0) s_over = 0;
    lds_barrier();
#pragma unroll
    for (uint32_t j = 0; j < BPT; ++j) {
        const uint32_t bj = threadIdx.x * BPT + j;
        if (bj >= nb) break;
        const uint32_t lim = bs_mine[j] >= cap ? 0u : min(c_mine[j], cap - bs_mine[j]);
        binfo[bj] = uint2{bj * cap + bs_mine[j] - soff[bj], soff[bj] + lim};
        if (lim < c_mine[j]) s_over = 1;  // benign race: every writer stores 1
    }
    lds_barrier();
    BSTAMP(3);
    const uint32_t total = soff[nb];
    BinItem* lvl_items = items + bp.item0[level];
    // in-capacity items: plain stores, back to back (with the overflow path's
    // returning atomics in the same loop the compiler waited for every
    // store's completion before the next)
    for (uint32_t k = threadIdx.x; k < total; k += kBinPts) {
        const BinItem it = stage[k];
        const uint2 bi = binfo[it.e >> 16];
        if (k < bi.y) {
            if constexpr (SC1)  // read by the same launch's accumulate workgroups
                __hip_atomic_store(reinterpret_cast<unsigned long long*>(lvl_items + k + bi.x),
                                   (unsigned long long)(it.e & 0xffffu) |
                                       ((unsigned long long)__builtin_bit_cast(uint32_t, it.v) << 32),
                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            else
                lvl_items[k + bi.x] = BinItem{it.e & 0xffffu, it.v};
        }
    }
    // Past a bin's capacity: the item's exact int64 counts go into the spill
    // image (integer atomics, so the sum does not depend on the arrival
    // order); the bin's first accumulate unit folds them in. A non-finite
    // item cannot be carried by the integers: it marks the bin instead.
    for (uint32_t k = threadIdx.x; s_over && k < total; k += kBinPts) {
        const BinItem it = stage[k];
        const uint32_t bin = it.e >> 16;
        const uint2 bi = binfo[bin];
        if (k >= bi.y) {
            const uint32_t vb = __builtin_bit_cast(uint32_t, it.v);
            if (((vb >> 10) & 31u) == 31u || ((vb >> 26) & 31u) == 31u) {
                atomicOr(spill_bad + bp.bin0[level] + bin, 1u);  // (an atomic: seen by the one-launch form's readers)
                if (nonfinite) atomicOr(nonfinite, 1);
            } else {
                const size_t e = (size_t)off0 + (size_t)bin * kBinEntries + (it.e & 0xffffu);
                atomicAdd(spill + 2 * e, (unsigned long long)half_fixed24(vb & 0xffffu));
                atomicAdd(spill + 2 * e + 1, (unsigned long long)half_fixed24(vb >> 16));
            }
        }
    }
    BSTAMP(4);
    BRSTAMP(9);
    }
}

template <uint32_t D, uint32_t NBMAX>
__global__ void __launch_bounds__(kBinPts, kBinWavesPerSimd * 256 / kBinPts)  // kBinWavesPerSimd waves per SIMD
k_grid_bwd_bin(const ngp_half* __restrict__ grad, const float* __restrict__ inputs,
               const int32_t* __restrict__ offsets, ngp_half* __restrict__ grad_grid, uint32_t B,
               uint32_t L, GridLevels lv, uint32_t gridtype, bool align_corners, uint32_t interp,
               InMap im, BinPlan bp, uint32_t* __restrict__ cursor, BinItem* __restrict__ items,
               int32_t grad_layout, int32_t* __restrict__ nonfinite, ngp_reduce::ReduceJobs rj, uint32_t nred,
               uint32_t* __restrict__ timing, BinLego next_batch, unsigned long long* __restrict__ spill,
               uint32_t* __restrict__ spill_bad, uint32_t* __restrict__ rows_out, ngp_reduce::DwProduct dw) {
    static_assert(kBinPts == 64 * ngp_reduce::kDwWaves, "a dW product workgroup is a bin workgroup");
    extern __shared__ __attribute__((aligned(16))) uint32_t bin_lds[];  // bin_lds_words<NBMAX>()
    bin_block<D, NBMAX, false>(grad, inputs, offsets, grad_grid, B, L, lv, gridtype, align_corners, interp, im, bp,
                               cursor, items, grad_layout, nonfinite, rj, nred, timing, next_batch, spill, spill_bad,
                               rows_out, blockIdx.x, blockIdx.y, gridDim.y, bin_lds, dw);
}

// Persistent accumulation: every workgroup reads all bins' counts, forms the
// work units (bin, segment of kSegItems items) and takes units blockIdx.x,
// blockIdx.x + gridDim.x, ... The last workgroup to have read the counts
// zeroes them for the next step. Per unit the items are summed EXACTLY in an
// LDS image of 64-bit fixed-point counts of 2^-24 (the fp16 quantum) with
// integer LDS atomics: ds_add_u64 costs ~15 cycles per wave-instruction on
// gfx950 against ~195 for ds_add_f32 / ds_pk_add_f16 (tools/lds_atomic_probe).
// All item loads of a batch are issued before its adds. The image is then
// written to the fp16 table when the unit is its bin's only one; the units of
// a bin with several add their images into the bin's int64 slot and the last
// to arrive writes the table. The first unit of a bin whose items ran past its
// capacity folds the bin's slice of the spill image in first. A non-finite item
// (inf / NaN: fp16 overflow under the loss scale) cannot be carried by the
// integers, so it marks the unit and the unit stores a NaN into its bin's
// first entry, which is what GradScaler's inf check looks for.
constexpr uint32_t kAccThreads = 512, kAccBatch = 8, kRetireGroups = 16;
// the accumulate's static LDS (the 64 KiB image and its small arrays), for the launch's occupancy choice
constexpr size_t kAccStaticLds = 66 * 1024 + 1024;
static_assert(kAccBatch > 0, "8 must be positive");
static_assert(kMaxLevels <= 64, "the accumulate finds a bin's level with one wave ballot");
static_assert(kBinEntries % kAccThreads == 0, "each flush thread owns whole entries (G > 0)");
// the int64 LDS image of one bin (+ the counts in dynamic LDS) fits a CU's 160 KB
static_assert(kBinEntries * 2 * sizeof(unsigned long long) <= 128 * 1024, "bin image exceeds LDS");
// Wave bins (round 7). In the live-row regime a hashed level's bin holds a few
// dozen to a few hundred items (Lego: ~120 of 4096 entries), and the
// workgroup image above spends most of its ~5.5 K cycles per unit zeroing,
// draining and flushing behind workgroup barriers, after a prologue that reads
// every bin's count (phase clocks, tools/accum_stamps.py). Here ONE WAVE owns
// a bin and needs no barrier and no prologue: it reads its own bin's count,
//   1. marks its items' entries in a 4096-bit LDS bitmap (ds_or),
//   2. ranks the marked entries (popcounts + one wave scan): entry e of the
//      bin gets a compact index among the bin's distinct entries,
//   3. adds every item's exact int64 2^-24 counts at its compact index
//      (ds_add_u64; integers, so the sum does not depend on the order),
//   4. walks the marked bits and stores each distinct entry's fp16 once.
// Same sums, same single rounding as the image path: the grads are bit-for-
// bit those of the workgroup image. A wave holds kWaveAcc distinct entries at a
// time; a bin with more runs steps 3-4 once per range of compact indices. LDS
// ops of one wave complete in issue order, so the phases need only the wave's
// own lgkmcnt waits. Used for the hashed levels of a cleared grad whose
// cursors the caller clears (the fused step); the dense levels (z-slab bins,
// thousands of items) keep the workgroup image.
constexpr uint32_t kWaveWords = kBinEntries / 32;                      // bitmap words per bin
constexpr uint32_t kWaveLdsUll = kBinEntries * 2 / (kAccThreads / 64);  // int64 words of LDS per wave
constexpr uint32_t kWaveAcc = (kWaveLdsUll - kWaveWords) / 2;          // distinct entries per pass (448)
#ifndef NGP_WAVE_Q
#define NGP_WAVE_Q 8
#endif
constexpr uint32_t kWaveQ = NGP_WAVE_Q;  // items per lane in flight (a bin of <= 64 kWaveQ items: one load round)
#ifndef NGP_WAVE_SPEC
#define NGP_WAVE_SPEC 0
#endif
constexpr uint32_t kWaveSpec = NGP_WAVE_SPEC;  // of them requested before the bin's count is known
static_assert(kWaveSpec <= kWaveQ, "speculative items are a prefix of the first round");
#ifndef NGP_WAVE_BINS
#define NGP_WAVE_BINS 1
#endif
constexpr bool kWaveBins = NGP_WAVE_BINS != 0;  // (0: the image path for every bin, A/B builds)
#ifndef NGP_ACC_IMAGE_WGS
#define NGP_ACC_IMAGE_WGS 128
#endif
constexpr uint32_t kAccImageWgs = NGP_ACC_IMAGE_WGS;  // workgroups of the image path beside the wave bins
#ifndef NGP_WAVE_MAX
#define NGP_WAVE_MAX 512
#endif
constexpr uint32_t kWaveMax = NGP_WAVE_MAX;  // mean items per hashed bin above which the image path takes every bin
#ifndef NGP_FUSED_BWD
#define NGP_FUSED_BWD 0
#endif
constexpr uint32_t kFusedBwd = NGP_FUSED_BWD;  // the one-launch grid backward (k_grid_bwd_fused): 1 tickets, 2 block roles
constexpr uint32_t kFusedYCap = 64;            // its point blocks per level (each loops over more)
// after the counters: the retire area (the accumulate's retire counters, the
// binned rows word, the one-launch form's ticket / done counters), cleared
// with the counters by a caller that clears them (NGP_GRID_CURSORS_EXTERNAL)
constexpr size_t kRetireBytes = 512;
constexpr uint32_t kFusedWords = 40;  // word of the retire area: ticket, finished count, error, -, done[level]
static_assert(kFusedWords + 4 + kMaxLevels <= kRetireBytes / 4, "the one-launch counters fit the retire area");
constexpr uint32_t kRowsWord = 32;           // word of the retire area (unused with external cursors): the binned rows
static_assert(kRowsWord > kRetireGroups && kRowsWord < 64, "the rows word lies in the 256-byte retire area, past its counters");
static_assert(kWaveWords == 128, "two bitmap words per lane");

NGP_DEV void lds_wait() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// Returns false (having done nothing) in the dense regime: rows_seen (loaded
// by the caller, waited for only after this bin's first loads) > rows_max.
template <bool SC1>
NGP_DEV bool wave_bin(uint32_t rows_seen, uint32_t rows_max, uint32_t gb, uint32_t level, uint32_t lbin, uint32_t cap, uint32_t item0,
                      uint32_t off0, uint32_t off1, const uint32_t* __restrict__ cursor,
                      const BinItem* __restrict__ items, ngp_half* __restrict__ grad_grid,
                      int32_t* __restrict__ nonfinite, unsigned long long* __restrict__ spill,
                      uint32_t* __restrict__ spill_bad, uint32_t* bm, uint32_t* pre, unsigned long long* sums,
                      uint32_t lane) {
    constexpr uint32_t C = 2;
    const uint64_t* src = reinterpret_cast<const uint64_t*>(items + item0 + (size_t)lbin * cap);
    // the first kWaveSpec x 64 item slots may be requested beside the count
    // (slots past the count hold stale items and are masked below; clamped to
    // the bin's capacity, so every address is the bin's own), the rest of the
    // first round once the count is known. All kWaveQ x 64 up front read 2.9x
    // the live items' bytes in the trained regime (PMC, r07ev); 0, 2 and 8
    // measured the same time (r07r), so none are speculative by default.
    uint64_t it[kWaveQ];
#pragma unroll
    for (uint32_t q = 0; q < kWaveSpec; ++q) it[q] = ld_u64<SC1>(src + min(q * 64 + lane, cap - 1u));
    const uint32_t raw = ld_u32<SC1>(cursor + gb);
    if (__builtin_amdgcn_readfirstlane(rows_seen) > rows_max) return false;  // (its wait after this bin's loads)
    STAMP(11, raw ? __builtin_amdgcn_s_memtime() : 0ull);
    if (raw == 0) return true;
    WSTAMP(0, (unsigned long long)min(raw, cap) | ((unsigned long long)level << 32) | ((unsigned long long)(raw > cap) << 40));
    WSTAMP(1, __builtin_amdgcn_s_memtime());
    const uint32_t n = min(raw, cap);
    const bool spilled = raw > cap;
#pragma unroll
    for (uint32_t q = kWaveSpec; q < kWaveQ; ++q) {
        const uint32_t k = q * 64 + lane;
        it[q] = k < n ? ld_u64<SC1>(src + k) : ~0ull;
    }
    const uint32_t e0 = lbin * kBinEntries;
    const uint32_t ne = min(kBinEntries, off1 - off0 - e0);
    const size_t ebase = (size_t)off0 + e0;
    ngp_half2* tbl = reinterpret_cast<ngp_half2*>(grad_grid + ebase * C);
    unsigned long long* sp = spill + 2 * ebase;
    // a bin of at most 64 kWaveQ items stays in registers; a larger one is
    // read again in each step (L2-warm)
    const bool one = n <= 64 * kWaveQ;
    auto load = [&](uint32_t k0) {
#pragma unroll
        for (uint32_t q = 0; q < kWaveQ; ++q) {
            const uint32_t k = k0 + q * 64 + lane;
            it[q] = k < n ? ld_u64<SC1>(src + k) : ~0ull;
        }
    };
    auto mask = [&]() {
#pragma unroll
        for (uint32_t q = 0; q < kWaveQ; ++q)
            if (q * 64 + lane >= n) it[q] = ~0ull;
    };
    // 1. bitmap of the bin's entries
    bool bad = false;
    for (uint32_t k0 = 0; k0 < n; k0 += 64 * kWaveQ) {
        if (k0) load(k0);
        else mask();
#pragma unroll
        for (uint32_t q = 0; q < kWaveQ; ++q) {
            if (it[q] == ~0ull) continue;
            const uint32_t e = (uint32_t)it[q] & (kBinEntries - 1), v = (uint32_t)(it[q] >> 32);
            bad |= ((v >> 10) & 31u) == 31u || ((v >> 26) & 31u) == 31u;
            atomicOr(&bm[e >> 5], 1u << (e & 31));
        }
    }
    if (spilled) {  // entries past the bin's capacity went to the spill image (rare)
        for (uint32_t e = lane; e < ne; e += 64) {
            const ulonglong2 x = ld_u64x2<SC1>(sp + 2 * e);
            if (x.x | x.y) atomicOr(&bm[e >> 5], 1u << (e & 31));
        }
        if (lane == 0 && ld_u32<SC1>(spill_bad + gb)) {
            bad = true;
            spill_bad[gb] = 0u;
        }
    }
    lds_wait();
    STAMP(12, __builtin_amdgcn_s_memtime());
    // 2. compact index of each marked entry: prefix of the popcounts
    const uint32_t w0 = bm[2 * lane], w1 = bm[2 * lane + 1];
    const uint32_t c0 = (uint32_t)__popc(w0), cnt = c0 + (uint32_t)__popc(w1);
    const uint32_t incl = ngp_dpp::scan_incl_u32(cnt);
    const uint32_t distinct = __builtin_amdgcn_readlane(incl, 63);
    pre[2 * lane] = incl - cnt;
    pre[2 * lane + 1] = incl - cnt + c0;
    lds_wait();
    auto cidx = [&](uint32_t e) {  // compact index of a marked entry
        const uint32_t w = bm[e >> 5];
        return pre[e >> 5] + (uint32_t)__popc(w & ((1u << (e & 31)) - 1u));
    };
    const bool unit_bad = __ballot(bad) != 0;
    const float q24 = 1.0f / 16777216.0f;
    bool inf_out = false;
    auto out_of = [&](const ulonglong2& xs, bool& store) {
        const int64_t x0 = (int64_t)xs.x, x1 = (int64_t)xs.y;
        store = !unit_bad && (x0 != 0 || x1 != 0);
        const ngp_half2 o{(ngp_half)((float)x0 * q24), (ngp_half)((float)x1 * q24)};
        if (store) inf_out |= !__builtin_isfinite((float)o[0]) || !__builtin_isfinite((float)o[1]);
        return o;
    };
    if (one && !spilled && distinct <= kWaveAcc) {
        // the common case: every item in registers, one range of sums. Each
        // item stores its entry's sum (items of one entry store the same
        // value); all LDS reads before the stores, no store in a loop (the
        // compiler waits for a store's data before reusing its registers)
        uint32_t ci[kWaveQ];
#pragma unroll
        for (uint32_t q = 0; q < kWaveQ; ++q)
            ci[q] = it[q] == ~0ull ? 0xffffffffu : cidx((uint32_t)it[q] & (kBinEntries - 1));
#pragma unroll
        for (uint32_t q = 0; q < kWaveQ; ++q) {
            if (ci[q] == 0xffffffffu) continue;
            const uint32_t v = (uint32_t)(it[q] >> 32);
            atomicAdd(&sums[2 * ci[q]], (unsigned long long)half_fixed24(v & 0xffffu));
            atomicAdd(&sums[2 * ci[q] + 1], (unsigned long long)half_fixed24(v >> 16));
        }
        lds_wait();
        ulonglong2 xs[kWaveQ];
#pragma unroll
        for (uint32_t q = 0; q < kWaveQ; ++q)
            xs[q] = ci[q] == 0xffffffffu ? ulonglong2{0ull, 0ull} : reinterpret_cast<const ulonglong2*>(sums)[ci[q]];
        lds_wait();  // every read is done before any clear
#pragma unroll
        for (uint32_t q = 0; q < kWaveQ; ++q)
            if (ci[q] != 0xffffffffu) reinterpret_cast<ulonglong2*>(sums)[ci[q]] = ulonglong2{0ull, 0ull};
#pragma unroll
        for (uint32_t q = 0; q < kWaveQ; ++q) {
            bool store;
            const ngp_half2 o = out_of(xs[q], store);
            if (store) tbl[(uint32_t)it[q] & (kBinEntries - 1)] = o;
        }
    } else {
        for (uint32_t r0 = 0; r0 < distinct; r0 += kWaveAcc) {
            // 3. exact sums of this range's entries
            for (uint32_t k0 = 0; k0 < n; k0 += 64 * kWaveQ) {
                if (!one || r0 > 0) load(k0);
#pragma unroll
                for (uint32_t q = 0; q < kWaveQ; ++q) {
                    if (it[q] == ~0ull) continue;
                    const uint32_t e = (uint32_t)it[q] & (kBinEntries - 1), v = (uint32_t)(it[q] >> 32);
                    const uint32_t i = cidx(e) - r0;
                    if (i >= kWaveAcc) continue;
                    atomicAdd(&sums[2 * i], (unsigned long long)half_fixed24(v & 0xffffu));
                    atomicAdd(&sums[2 * i + 1], (unsigned long long)half_fixed24(v >> 16));
                }
            }
            if (spilled) {
                for (uint32_t e = lane; e < ne; e += 64) {
                    const ulonglong2 x = ld_u64x2<SC1>(sp + 2 * e);
                    if (!(x.x | x.y)) continue;
                    const uint32_t i = cidx(e) - r0;
                    if (i >= kWaveAcc) continue;
                    atomicAdd(&sums[2 * i], x.x);
                    atomicAdd(&sums[2 * i + 1], x.y);
                }
            }
            lds_wait();
            // 4. each distinct entry of the range once: the lane owning its
            // bitmap word reads the sums and stores the fp16 pair, kFlushB at
            // a time (all reads of a batch before its stores)
            constexpr uint32_t kFlushB = 8;
#pragma unroll
            for (uint32_t h = 0; h < 2; ++h) {
                uint32_t w = h ? w1 : w0;
                uint32_t rank = h ? pre[2 * lane] + c0 : pre[2 * lane];
                while (w) {
                    uint32_t ent[kFlushB];
                    ulonglong2 xs[kFlushB];
#pragma unroll
                    for (uint32_t j = 0; j < kFlushB; ++j) {
                        ent[j] = 0xffffffffu;
                        xs[j] = ulonglong2{0ull, 0ull};
                        if (!w) continue;
                        const uint32_t bt = (uint32_t)__builtin_ctz(w);
                        w &= w - 1u;
                        const uint32_t i = rank++ - r0;
                        if (i >= kWaveAcc) continue;
                        ent[j] = (2 * lane + h) * 32 + bt;
                        xs[j] = reinterpret_cast<const ulonglong2*>(sums)[i];
                    }
#pragma unroll
                    for (uint32_t j = 0; j < kFlushB; ++j) {
                        bool store;
                        const ngp_half2 o = out_of(xs[j], store);
                        if (store && ent[j] != 0xffffffffu) tbl[ent[j]] = o;
                    }
                }
            }
            lds_wait();  // every read of the range is done before any clear
            for (uint32_t i = lane; i < min(kWaveAcc, distinct - r0); i += 64)
                reinterpret_cast<ulonglong2*>(sums)[i] = ulonglong2{0ull, 0ull};
        }
    }
    STAMP(13, __builtin_amdgcn_s_memtime());
    if (spilled)  // folded: clear the bin's slice of the spill image for the next call
        for (uint32_t e = lane; e < ne; e += 64) reinterpret_cast<ulonglong2*>(sp)[e] = ulonglong2{0ull, 0ull};
    bm[2 * lane] = 0u;
    bm[2 * lane + 1] = 0u;
    lds_wait();
    if (unit_bad && !nonfinite && lane == 0) tbl[0] = ngp_half2{(ngp_half)__builtin_nanf(""), (ngp_half)0.0f};
    if (nonfinite && (__ballot(inf_out) != 0 || unit_bad) && lane == 0) atomicOr(nonfinite, 1);
    WSTAMP(2, __builtin_amdgcn_s_memtime());
    WSTAMP(3, distinct);
    return true;
}

// ZEROED (the fused step: NGP_GRID_GRAD_ZEROED) drops the read-back of owned
// slices (non-fresh owners occur only with a grad that was not zeroed) and the
// registers it holds.
// The one-launch form's synchronisation (k_grid_bwd_fused): each bin
// workgroup adds 1 to done[level] once its items are stored; an accumulate
// workgroup waits for the levels it reads. err: a wait that ran out (bounded).
struct FusedSync {
    uint32_t* done;        // [nlev] bin workgroups finished, per level (zero before the launch)
    uint32_t per_level;    // bin workgroups per level
    uint32_t* err;         // set to 1 when a bounded wait ran out
    uint32_t* opened;      // 1 once the launch-timing ring entry is open (ticket 0's workgroup)
};
// Poll (one lane) until *p >= need; bounded (~0.1 s), then flags err.
NGP_DEV void wait_at_least(const uint32_t* p, uint32_t need, uint32_t* err) {
    for (uint32_t it = 0; it < (1u << 17); ++it) {
        if (__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= need) return;
        __builtin_amdgcn_s_sleep(16);
    }
    if (err) atomicOr(err, 1u);
}

template <bool ZEROED, bool FUSED>
NGP_DEV void accum_block(const int32_t* __restrict__ offsets, ngp_half* __restrict__ grad_grid, const BinPlan& bp,
                         uint32_t* __restrict__ cursor, uint32_t* __restrict__ retire,
                         const BinItem* __restrict__ items, int32_t* __restrict__ nonfinite,
                         bool external, unsigned long long* __restrict__ msums,
                         uint32_t* __restrict__ marrive, uint32_t* __restrict__ timing,
                         int32_t* __restrict__ reset_counter, unsigned long long* __restrict__ spill,
                         uint32_t* __restrict__ spill_bad, uint32_t wave_bins0, uint32_t nimg,
                         const uint32_t* __restrict__ rows_in, uint32_t wave_rows_max, uint32_t bid, uint32_t nblk,
                         unsigned long long* acc, uint32_t* dyn, const FusedSync& fs) {
    constexpr uint32_t C = 2, NW = kAccThreads / 64;
    // [entry][channel]; a channel-planar image (8-byte lane stride for the
    // 64-bit atomics instead of 16) measured the same
    auto acc_entry = [&](uint32_t e) { return reinterpret_cast<const ulonglong2*>(acc)[e]; };
    __shared__ uint32_t wsum[NW];
    __shared__ uint32_t s_last, s_bad;
    // bins [wave_bins0, total) go one per wave (wave_bin) to the workgroups
    // from nimg on; the first nimg workgroups run the image path over the
    // bins before wave_bins0 (wave_bins0 = total: every workgroup, every bin).
    // Dense regime: more rows than wave_rows_max (the rows this call's bin
    // launch binned, *rows_in) put ~kWaveMax items or more in a hashed bin,
    // where the image path is faster: every workgroup then runs it over every
    // bin. The row count is loaded beside each role's first loads.
    uint32_t nbins = min(wave_bins0, bp.total_bins);
    const bool waves = nbins < bp.total_bins;
    const uint32_t rows_seen = waves && rows_in ? *rows_in : 0u;
    bool wave_role = waves && bid >= nimg;
    STAMP(0, __builtin_amdgcn_s_memtime());
    RSTAMP(60);
    // the plan's per-level arrays, indexed per lane below: kernel arguments
    // indexed by a varying value are memory loads, so keep a copy in LDS
    __shared__ uint32_t s_bin0[kMaxLevels + 1], s_cap[kMaxLevels], s_item0[kMaxLevels], s_off[kMaxLevels + 1];
    __shared__ uint32_t s_mslot0[kMaxLevels];
    __shared__ uint32_t s_lastunit;
    const uint32_t t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const uint32_t nlev = bp.nlev;
    // the sample counter of the batch whose backward this is, once every
    // kernel that reads it has finished (the bin launch drew the next batch)
    if (reset_counter && bid == 0 && t < 2) reset_counter[t] = 0;
    uint32_t ngr_img = nimg;  // workgroups of the image path
    if (wave_role) {
        // no plan copy and no barrier: a wave's level and plan entries are
        // wave-uniform, read from the kernel arguments with scalar loads
        unsigned long long* wl = acc + wv * kWaveLdsUll;  // this wave's 8 KB: bitmap, prefix, sums
        for (uint32_t i = lane; i < kWaveLdsUll / 2; i += 64) reinterpret_cast<ulonglong2*>(wl)[i] = ulonglong2{0ull, 0ull};
        STAMP(10, __builtin_amdgcn_s_memtime());
        const uint32_t nw = (nblk - nimg) * NW;
        uint32_t lv = 0, lv_ready = 0xffffffffu;
        for (uint32_t gb = nbins + (bid - nimg) * NW + wv; gb < bp.total_bins; gb += nw) {
            gb = __builtin_amdgcn_readfirstlane(gb);
            while (lv + 1 < nlev && gb >= bp.bin0[lv + 1]) ++lv;
            if constexpr (FUSED) {  // this level's bin workgroups have stored their items
                if (lv != lv_ready && __builtin_amdgcn_readfirstlane(rows_seen) <= wave_rows_max) {
                    if (lane == 0) wait_at_least(fs.done + lv, fs.per_level, fs.err);
                    lv_ready = lv;
                }
            }
            if (!wave_bin<FUSED>(rows_seen, wave_rows_max, gb, lv, gb - bp.bin0[lv], bp.cap[lv], bp.item0[lv], bp.off[lv], bp.off[lv + 1],
                          cursor, items, grad_grid, nonfinite, spill, spill_bad, reinterpret_cast<uint32_t*>(wl),
                          reinterpret_cast<uint32_t*>(wl) + kWaveWords, wl + kWaveWords, lane))
                break;
        }
        if (__builtin_amdgcn_readfirstlane(rows_seen) > wave_rows_max) {  // every wave saw the same row count
            wave_role = false;
            nbins = bp.total_bins;
            ngr_img = nblk;
        } else {
            STAMP(14, __builtin_amdgcn_s_memtime());
            __syncthreads();  // the workgroup's end below is its last wave's
        }
    }
    if (!wave_role) {
    // the first group of this thread's bin counts (step 1 below) is loaded
    // before anything else: its round trip overlaps the plan's LDS copy
    constexpr uint32_t kStep1Loads = 4;
    // (sized for every bin: the same ownership whichever bins this call takes)
    const uint32_t per = (bp.total_bins + kAccThreads - 1) / kAccThreads;
    uint32_t cv0[kStep1Loads];
#pragma unroll
    for (uint32_t j = 0; j < kStep1Loads; ++j) {
        const uint32_t b = t * per + j;
        cv0[j] = !FUSED && j < per && b < bp.total_bins ? cursor[b] : 0u;
    }
    if (waves && ngr_img == nimg && rows_seen > wave_rows_max) {  // dense regime (decided after the loads above are issued)
        nbins = bp.total_bins;
        ngr_img = nblk;
    }
    if constexpr (FUSED) {
        // the levels of this role's bins have stored their items (the dense
        // regime: every level), then the counts
        if (t < 64) {
            for (uint32_t l = 0; l < bp.nlev; ++l) {
                if (bp.bin0[l] >= nbins) break;
                if (t == 0) wait_at_least(fs.done + l, fs.per_level, fs.err);
            }
        }
        __syncthreads();
#pragma unroll
        for (uint32_t j = 0; j < kStep1Loads; ++j) {
            const uint32_t b = t * per + j;
            cv0[j] = j < per && b < bp.total_bins ? ld_u32<true>(cursor + b) : 0u;
        }
    }
    // (after the regime is known: nbins is final here; the host sized the
    // dynamic LDS for every bin whenever the dense regime can occur)
    uint32_t* upre = dyn;              // [nbins + 1] first unit of each bin
    uint32_t* bn = dyn + nbins + 1;    // [nbins] items of each bin (clipped at its capacity)
    if (t <= nlev) {
        s_bin0[t] = t < nlev ? bp.bin0[t] : bp.total_bins;
        s_off[t] = bp.off[t];  // (the plan's host copy: no global load ahead of the first barrier)
        if (t < nlev) {
            s_cap[t] = bp.cap[t];
            s_item0[t] = bp.item0[t];
            s_mslot0[t] = bp.mslot0[t];
        }
    }
    // the image starts zeroed (while the counts are in flight)
    for (uint32_t i = t; i < kBinEntries * C / 2; i += kAccThreads)
        reinterpret_cast<uint4*>(acc)[i] = uint4{0u, 0u, 0u, 0u};
    if (t == 0) s_bad = 0;
    lds_barrier();
    auto level_of = [&](uint32_t b) {  // last level whose first bin is <= b (binary lifting)
        uint32_t l = 0;
#pragma unroll
        for (uint32_t s = kMaxLevels / 2; s; s >>= 1)
            if (l + s < nlev && b >= s_bin0[l + s]) l += s;
        return l;
    };

    // 1. units per bin, exclusive prefix (thread t owns bins [t*per, t*per + per)).
    // The counts are loaded kStep1Loads at a time, all before their use (one
    // round trip per group instead of one per bin).
    uint32_t mine = 0;
    uint32_t level = t * per < nbins ? level_of(t * per) : 0;
    for (uint32_t j0 = 0; j0 < per; j0 += kStep1Loads) {
        uint32_t cv[kStep1Loads];
#pragma unroll
        for (uint32_t j = 0; j < kStep1Loads; ++j) {
            const uint32_t b = t * per + j0 + j;
            cv[j] = j0 == 0 ? cv0[j] : j0 + j < per && b < nbins ? ld_u32<FUSED>(cursor + b) : 0u;
        }
#pragma unroll
        for (uint32_t j = 0; j < kStep1Loads; ++j) {
            const uint32_t b = t * per + j0 + j;
            if (j0 + j >= per || b >= nbins) break;
            while (level + 1 < nlev && b >= s_bin0[level + 1]) ++level;
            const uint32_t n = min(cv[j], s_cap[level]);
            bn[b] = n | (cv[j] > s_cap[level] ? 0x80000000u : 0u);  // top bit: items spilled
            const uint32_t nu = (n + kSegItems - 1) / kSegItems;      // n: the clipped count
            upre[b] = nu;
            mine += nu;
        }
    }
    const uint32_t incl = ngp_dpp::scan_incl_u32(mine);
    if (lane == 63) wsum[wv] = incl;
    __syncthreads();
    uint32_t run = incl - mine, total = 0;
#pragma unroll
    for (uint32_t w = 0; w < NW; ++w) {
        run += w < wv ? wsum[w] : 0u;
        total += wsum[w];
    }
    for (uint32_t j = 0; j < per; ++j) {
        const uint32_t b = t * per + j;
        if (b >= nbins) break;
        const uint32_t u = upre[b];
        upre[b] = run;
        run += u;
    }
    if (t == 0) upre[nbins] = total;
    STAMP(1, __builtin_amdgcn_s_memtime());
    // 2. retire: once every workgroup holds the counts, the last one zeroes
    // them for the next step. Two-level counter (kRetireGroups group counters,
    // then one), so no address takes more than ~gridDim / kRetireGroups
    // atomics: 512 workgroups through one counter cost ~10 us; this one still
    // ~7 us (phase clocks, tools/accum_stamps.py), so a caller that clears the
    // counters itself (NGP_GRID_CURSORS_EXTERNAL: the fused step's head
    // kernel) skips it.
    if (!external && t == 0) {
        __threadfence();
        const uint32_t grp = bid % kRetireGroups;
        const uint32_t members = nblk / kRetireGroups + (grp < nblk % kRetireGroups ? 1u : 0u);
        s_last = 0;
        if (atomicAdd(&retire[1 + grp], 1u) == members - 1) {
            retire[1 + grp] = 0;
            const uint32_t groups = min(nblk, kRetireGroups);
            s_last = atomicAdd(&retire[0], 1u) == groups - 1;
        }
    }
    __syncthreads();
    if (!external && s_last) {
        for (uint32_t b = t; b < nbins; b += kAccThreads) cursor[b] = 0;
        if (t == 0) retire[0] = 0;
    }
    STAMP(2, __builtin_amdgcn_s_memtime());
    [[maybe_unused]] uint32_t nstamp = 0;

    // 3. units. The first item batch of a unit and, for a single-owner unit,
    // its slice of the table are loaded one unit ahead (while the previous
    // unit does its LDS adds and writes), hiding the memory latency.
    // No bool members: with them the struct lived in scratch memory (a
    // private-segment load and store per unit, waited on like any other).
    // flags; fresh: the table slice is known to be zero; multi: one of several
    // units of a bin, finished through the bin's int64 slot; spill: the bin's
    // first unit, and items of the bin went to the spill image
    constexpr uint32_t kOwner = 1, kFresh = 2, kMulti = 4, kSpill = 8;
    struct Unit {
        uint32_t level, lbin, gb, s0, s1, ne, flags, slot, nunits;
        const uint64_t* src;
        ngp_half2* tbl;
    };
    // The unit's bin: the last bin whose first unit is <= u, found 64 ways
    // per round (two dependent LDS reads for up to 4096 bins; a binary
    // search took ~11), and its level by one ballot over the level starts.
    auto locate = [&](uint32_t u) {
        uint32_t lo = 0, n = nbins;
        while (n > 1) {
            const uint32_t stride = (n + 63) / 64, k = lane * stride;
            const uint64_t mk = __ballot(k < n && upre[lo + k] <= u);  // lane 0 always qualifies
            const uint32_t L = 63u - (uint32_t)__builtin_clzll(mk);
            lo += L * stride;
            n = min(stride, n - L * stride);
        }
        Unit r;
        const uint32_t gb = lo, seg = u - upre[gb];
        r.nunits = upre[gb + 1] - upre[gb];
        const bool owner = r.nunits == 1;
        r.level = 63u - (uint32_t)__builtin_clzll(__ballot(lane < nlev && s_bin0[lane] <= gb));
        r.lbin = gb - s_bin0[r.level];
        // several units: the bin's count passed kSegItems, so its capacity
        // did and the plan gave its level int64 slots
        r.slot = s_mslot0[r.level] == kNoSlot ? kNoSlot : s_mslot0[r.level] + r.lbin;
        r.flags = (owner ? kOwner : kMulti) | (owner && ZEROED ? kFresh : 0u) |
                  ((bn[gb] >> 31) != 0 && seg == 0 ? kSpill : 0u);
        r.gb = gb;
        r.s0 = seg * kSegItems;
        r.s1 = min(bn[gb] & 0x7fffffffu, r.s0 + kSegItems);
        r.src = reinterpret_cast<const uint64_t*>(items + s_item0[r.level] + (size_t)r.lbin * s_cap[r.level]);
        const uint32_t off0 = s_off[r.level];
        const uint32_t hs = s_off[r.level + 1] - off0;
        const uint32_t e0 = r.lbin * kBinEntries;
        r.ne = min(kBinEntries, hs - e0);  // a multiple of 8 (offsets are)
        r.tbl = reinterpret_cast<ngp_half2*>(grad_grid + ((size_t)off0 + e0) * C);
        return r;
    };
    constexpr uint32_t G = kBinEntries / kAccThreads;  // table entries per thread (flush)
    auto load_batch = [&](const Unit& w, uint32_t k0, uint64_t (&it)[kAccBatch]) {
#pragma unroll
        for (uint32_t q = 0; q < kAccBatch; ++q) {
            const uint32_t k = k0 + q * kAccThreads + t;
            it[q] = k < w.s1 ? ld_u64<FUSED>(w.src + k) : ~0ull;
        }
    };
    // Only a non-fresh owner reads its slice back. No select on the loaded
    // value here: consuming it (a `fresh ? 0 : load` select) made the compiler
    // wait vmcnt(0) -- for the whole item prefetch issued just before -- right
    // after issuing it (phase clocks: ~6 K cycles per unit, tools/accum_stamps.py).
    auto load_old = [&](const Unit& w, uint32_t (&old)[G]) {
        if (ZEROED || (w.flags & (kOwner | kFresh)) != kOwner) return;
#pragma unroll
        for (uint32_t j = 0; j < G; ++j) {
            const uint32_t e = j * kAccThreads + t;
            if (e < w.ne) old[j] = reinterpret_cast<const uint32_t*>(w.tbl)[e];
        }
    };
    uint64_t it[kAccBatch];
    uint32_t old[G] = {};
    Unit cur{};
    // Unit order: round k gives unit k * grid + blockIdx.x, except the last,
    // partial round, which is dealt in reverse (grid - 1 - blockIdx.x). The
    // units run in bin order, so round 0's first workgroups hold the coarse
    // levels' long units (up to 4x the items of a fine-level unit); dealt
    // forward they also got a round-2 unit and finished last.
    const uint32_t ngr = ngr_img, full = total / ngr;
    auto unit_at = [&](uint32_t k) {  // this workgroup's k-th unit, or total (none)
        const uint32_t uk = k < full ? k * ngr + bid : full * ngr + (ngr - 1 - bid);
        return k <= full && uk < total ? uk : total;
    };
    uint32_t u = unit_at(0);
    if (u < total) {
        cur = locate(u);
        load_batch(cur, cur.s0, it);
        load_old(cur, old);
    }
    // Sparse units (a cleared grad's owner with at most kSparseMax items: the
    // 2^22-entry levels' bins, the Lego's levels 5-6) flush per ITEM instead
    // of per entry: each lane reads its items' sums, stores them (items of
    // one entry store the same value) and, after a barrier, clears just
    // those entries -- no 4096-entry flush and no zeroing pass for the next
    // unit. The entries are kept in ent[] (the prefetch overwrites it[]).
    constexpr uint32_t kSparseQ = 4, kSparseMax = kSparseQ * kAccThreads;
    static_assert(kSparseQ <= kAccBatch, "a sparse unit is one item batch");
    bool need_zero = false;  // the image holds entries no flush cleared (zeroed at the start)
    for (uint32_t k = 0; u < total; ++k) {
        // (clearing each entry in the flush right after reading it, by the
        // same lane -- no zeroing pass -- gave wrong sums on the GPU; the
        // sparse flush below clears only after a barrier)
        if (need_zero) {
            for (uint32_t i = t; i < kBinEntries * C / 2; i += kAccThreads)
                reinterpret_cast<uint4*>(acc)[i] = uint4{0u, 0u, 0u, 0u};
            if (t == 0) s_bad = 0;
            lds_barrier();
        }
        [[maybe_unused]] const uint32_t sb = 4 + 5 * min(nstamp, 11u);
        STAMP(sb, __builtin_amdgcn_s_memtime());
        const size_t ebase = (size_t)s_off[cur.level] + (size_t)cur.lbin * kBinEntries;
        STAMP(sb + 3, (cur.s1 - cur.s0) | ((uint64_t)(cur.flags & kOwner) << 32) | ((uint64_t)cur.level << 40));
        bool bad = false;
        for (uint32_t k0 = cur.s0;;) {
#pragma unroll
            for (uint32_t q = 0; q < kAccBatch; ++q) {
                if (it[q] == ~0ull) continue;
                const uint32_t e = (uint32_t)it[q], v = (uint32_t)(it[q] >> 32);
                bad |= ((v >> 10) & 31u) == 31u || ((v >> 26) & 31u) == 31u;
                atomicAdd(&acc[e * C], (unsigned long long)half_fixed24(v & 0xffffu));
                atomicAdd(&acc[e * C + 1], (unsigned long long)half_fixed24(v >> 16));
            }
            k0 += kAccThreads * kAccBatch;
            if (k0 >= cur.s1) break;
            load_batch(cur, k0, it);
        }
        STAMP(sb + 1, __builtin_amdgcn_s_memtime());
        if (cur.flags & kSpill) {
            // the bin's spilled items: add its slice of the spill image (one
            // entry per lane, after every item add has landed) and clear it
            lds_barrier();
            unsigned long long* sp = spill + 2 * ebase;
#pragma unroll 1
            for (uint32_t e = t; e < cur.ne; e += kAccThreads) {
                const ulonglong2 x = ld_u64x2<FUSED>(sp + 2 * e);
                if (x.x | x.y) {
                    acc[e * C] += x.x;
                    acc[e * C + 1] += x.y;
                    reinterpret_cast<ulonglong2*>(sp)[e] = ulonglong2{0ull, 0ull};
                }
            }
            if (t == 0 && ld_u32<FUSED>(spill_bad + cur.gb)) {
                bad = true;
                spill_bad[cur.gb] = 0u;
            }
        }
        const bool sparse = (cur.flags & (kFresh | kSpill)) == kFresh && cur.s1 - cur.s0 <= kSparseMax;
        uint32_t ent[kSparseQ];  // sparse: this lane's items' entries (0xffffffff: none)
#pragma unroll
        for (uint32_t q = 0; q < kSparseQ; ++q) ent[q] = it[q] == ~0ull ? 0xffffffffu : (uint32_t)it[q];
        uint32_t old_cur[G];
#pragma unroll
        for (uint32_t j = 0; j < G; ++j) old_cur[j] = old[j];
        // prefetch the next unit
        const uint32_t un = unit_at(k + 1);
        Unit nxt = cur;
        if (un < total) {
            nxt = locate(un);
            load_batch(nxt, nxt.s0, it);
            load_old(nxt, old);
        }
        if (__ballot(bad)) s_bad = 1;  // benign race: every writer stores 1
        lds_barrier();
        STAMP(sb + 4, __builtin_amdgcn_s_memtime());
        const bool unit_bad = s_bad != 0;
        const float q24 = 1.0f / 16777216.0f;
        bool inf_out = false;  // a stored grad is inf/nan (GradScaler's check, when `nonfinite` is given)
        if (sparse) {
            ulonglong2 xs[kSparseQ];
#pragma unroll
            for (uint32_t q = 0; q < kSparseQ; ++q)
                xs[q] = ent[q] != 0xffffffffu ? acc_entry(ent[q]) : ulonglong2{0ull, 0ull};
#pragma unroll
            for (uint32_t q = 0; q < kSparseQ; ++q) {
                const int64_t x0 = (int64_t)xs[q].x, x1 = (int64_t)xs[q].y;
                // (a bad unit stores only its NaN marker below: an item store
                // to entry 0 from another lane would race with it)
                if (unit_bad || ent[q] == 0xffffffffu || (x0 == 0 && x1 == 0)) continue;
                const ngp_half2 n{(ngp_half)((float)x0 * q24), (ngp_half)((float)x1 * q24)};
                inf_out |= !__builtin_isfinite((float)n[0]) || !__builtin_isfinite((float)n[1]);
                cur.tbl[ent[q]] = n;
            }
            lds_barrier();  // every lane's reads are done before any entry is cleared
#pragma unroll
            for (uint32_t q = 0; q < kSparseQ; ++q)
                if (ent[q] != 0xffffffffu) reinterpret_cast<ulonglong2*>(acc)[ent[q]] = ulonglong2{0ull, 0ull};
            if (t == 0) s_bad = 0;  // read above, before the barrier
            need_zero = false;
        } else if (cur.flags & kFresh) {
            need_zero = true;
            // the common case: the unit owns its slice of a cleared grad. All of
            // the lane's LDS reads first, then the stores. Nothing here consumes
            // a global load, so no wait on the next unit's prefetched items (with
            // the old values in the loop below, the compiler waited vmcnt(0) --
            // every outstanding load and store -- before each entry).
            ulonglong2 xs[G];
#pragma unroll
            for (uint32_t j = 0; j < G; ++j) {
                const uint32_t e = j * kAccThreads + t;
                xs[j] = e < cur.ne ? acc_entry(e) : ulonglong2{0ull, 0ull};
            }
#pragma unroll
            for (uint32_t j = 0; j < G; ++j) {
                const int64_t x0 = (int64_t)xs[j].x, x1 = (int64_t)xs[j].y;
                if (x0 == 0 && x1 == 0) continue;  // also every e >= ne
                const ngp_half2 n{(ngp_half)((float)x0 * q24), (ngp_half)((float)x1 * q24)};
                inf_out |= !__builtin_isfinite((float)n[0]) || !__builtin_isfinite((float)n[1]);
                cur.tbl[j * kAccThreads + t] = n;
            }
        } else if (cur.flags & kMulti) {
            need_zero = true;
            // one of several units of a bin: its exact partial sums go into the
            // bin's int64 slot (integer adds: the total does not depend on the
            // units' order), then the last unit to arrive takes the totals
            // (clearing the slot for the next call) and finishes the bin as an
            // owner would
            unsigned long long* sums = msums + (size_t)cur.slot * kBinEntries * C;
#pragma unroll 1
            for (uint32_t e = t; e < cur.ne; e += kAccThreads) {
                const ulonglong2 xx = acc_entry(e);
                if (xx.x) atomicAdd(sums + 2 * e, xx.x);
                if (xx.y) atomicAdd(sums + 2 * e + 1, xx.y);
            }
            __threadfence();  // this thread's adds are done before the workgroup arrives
            __syncthreads();
            if (t == 0) s_lastunit = atomicAdd(marrive + cur.slot, 1u) == cur.nunits - 1 ? 1u : 0u;
            __syncthreads();
            if (s_lastunit) {
                __threadfence();
                if (t == 0) marrive[cur.slot] = 0;
#pragma unroll 1
                for (uint32_t e = t; e < cur.ne; e += kAccThreads) {
                    const int64_t x0 = (int64_t)atomicExch(sums + 2 * e, 0ull);
                    const int64_t x1 = (int64_t)atomicExch(sums + 2 * e + 1, 0ull);
                    float o0 = 0.0f, o1 = 0.0f;  // a grad that was not zeroed: added to
                    if (!ZEROED && (x0 != 0 || x1 != 0)) {
                        const ngp_half2 o = cur.tbl[e];
                        o0 = (float)o[0];
                        o1 = (float)o[1];
                    }
                    const ngp_half2 n{(ngp_half)(o0 + (float)x0 * q24), (ngp_half)(o1 + (float)x1 * q24)};
                    inf_out |= !__builtin_isfinite((float)n[0]) || !__builtin_isfinite((float)n[1]);
                    if (x0 != 0 || x1 != 0) cur.tbl[e] = n;
                }
            }
        } else if (!ZEROED && (cur.flags & kOwner)) {
            need_zero = true;
            // one entry per lane per step: a lane reads its entry's two 8-byte
            // sums as one 16-byte LDS read (consecutive lanes, consecutive 16 B:
            // conflict-free) and stores the entry's half2 (256 B per wave)
#pragma unroll
            for (uint32_t j = 0; j < G; ++j) {
                const uint32_t e = j * kAccThreads + t;
                if (e >= cur.ne) continue;
                const ulonglong2 xx = acc_entry(e);
                const int64_t x0 = (int64_t)xx.x, x1 = (int64_t)xx.y;
                if (x0 == 0 && x1 == 0) continue;
                const ngp_half2 o = __builtin_bit_cast(ngp_half2, old_cur[j]);
                const ngp_half2 n{(ngp_half)((float)o[0] + (float)x0 * q24), (ngp_half)((float)o[1] + (float)x1 * q24)};
                inf_out |= !__builtin_isfinite((float)n[0]) || !__builtin_isfinite((float)n[1]);
                cur.tbl[e] = n;
            }
        }
        // a NaN grad marks a bad unit for a caller without the flag (a flagged
        // one reports below)
        if (unit_bad && !nonfinite && t == 0) cur.tbl[0] = ngp_half2{(ngp_half)__builtin_nanf(""), (ngp_half)0.0f};
        if (nonfinite && (__ballot(inf_out) != 0 || unit_bad) && (t & 63) == 0) atomicOr(nonfinite, 1);
        lds_barrier();  // the image is rezeroed by the next unit
        STAMP(sb + 2, __builtin_amdgcn_s_memtime());
        ++nstamp;
        STAMP(3, nstamp);
        cur = nxt;
        u = un;
    }
    }  // image role
    RSTAMP(61);
    // launch timing (NGP_GRID_TIMING): every workgroup stores its end in the
    // call's ring entry (one vector store each, no atomics, so the timed
    // kernel keeps its critical path); the host takes the latest
    if (timing && t == 0) {
        // (the one-launch form: level 0's first bin workgroup opened this
        // call's entry; wait for it before reading the call count)
        if constexpr (FUSED) wait_at_least(fs.opened, 1u, fs.err);
        const uint32_t c = (ld_u32<FUSED>(timing) - 1) % NGP_GRID_TIMING_RING;
        if (bid == 0) timing[kTimingHeads + c * 4 + 2] = nblk;
        if (bid < NGP_GRID_TIMING_MAX_WG)
            timing[kTimingEnds + c * NGP_GRID_TIMING_MAX_WG + bid] = (uint32_t)__builtin_amdgcn_s_memrealtime();
    }}

template <bool ZEROED>
__global__ void __launch_bounds__(kAccThreads, 4)  // 2 workgroups per CU: <= 128 VGPRs
k_grid_bin_accum(const int32_t* __restrict__ offsets, ngp_half* __restrict__ grad_grid, BinPlan bp,
                 uint32_t* __restrict__ cursor, uint32_t* __restrict__ retire,
                 const BinItem* __restrict__ items, int32_t* __restrict__ nonfinite,
                 bool external, unsigned long long* __restrict__ msums,
                 uint32_t* __restrict__ marrive, uint32_t* __restrict__ timing,
                 int32_t* __restrict__ reset_counter, unsigned long long* __restrict__ spill,
                 uint32_t* __restrict__ spill_bad, uint32_t wave_bins0, uint32_t nimg,
                 const uint32_t* __restrict__ rows_in, uint32_t wave_rows_max) {
    // [entry][channel]; a channel-planar image (8-byte lane stride for the
    // 64-bit atomics instead of 16) measured the same
    __shared__ __attribute__((aligned(16))) unsigned long long acc[kBinEntries * 2];
    extern __shared__ uint32_t dyn[];
    accum_block<ZEROED, false>(offsets, grad_grid, bp, cursor, retire, items, nonfinite, external, msums, marrive,
                               timing, reset_counter, spill, spill_bad, wave_bins0, nimg, rows_in, wave_rows_max,
                               blockIdx.x, gridDim.x, acc, dyn, FusedSync{});
}

// The grid backward as ONE launch (round 7; the fused step's configuration:
// cursors cleared by the caller, a zeroed grad, the wave bins). A workgroup
// takes a ticket: the first nlev x ycap tickets bin (level, point block), the
// next ones run the MLP dW reduce and the sampler columns, the rest
// accumulate. Tickets are taken in order by running workgroups, so when an
// accumulate workgroup waits on a level's done counter, every bin workgroup
// of that level holds a ticket and is running or finished: no wait depends
// on a workgroup that may not be resident (MI355X_MICROARCH.md: dispatch
// order is not promised). A hashed bin's wave starts as soon as its level's
// bin workgroups are done instead of after the whole bin launch and the
// launch boundary; the dense levels' image units after theirs. Items are
// stored and loaded `sc1`, the done counters are agent-scope atomics added
// after every storing wave's vmcnt(0) wait and a workgroup barrier.
template <uint32_t D, uint32_t NBMAX>
__global__ void __launch_bounds__(kAccThreads, 4)
k_grid_bwd_fused(const ngp_half* __restrict__ grad, const float* __restrict__ inputs,
                 const int32_t* __restrict__ offsets, ngp_half* __restrict__ grad_grid, uint32_t B,
                 uint32_t L, GridLevels lv, uint32_t gridtype, bool align_corners, uint32_t interp,
                 InMap im, BinPlan bp, uint32_t* __restrict__ cursor, BinItem* __restrict__ items,
                 int32_t grad_layout, int32_t* __restrict__ nonfinite, ngp_reduce::ReduceJobs rj, uint32_t nred,
                 uint32_t* __restrict__ timing, BinLego next_batch, unsigned long long* __restrict__ spill,
                 uint32_t* __restrict__ spill_bad, uint32_t* __restrict__ retire,
                 unsigned long long* __restrict__ msums, uint32_t* __restrict__ marrive,
                 int32_t* __restrict__ reset_counter, uint32_t wave_bins0, uint32_t nimg,
                 const uint32_t* __restrict__ rows_in, uint32_t wave_rows_max, uint32_t ycap, uint32_t nacc) {
    static_assert(kAccThreads == kBinPts, "one workgroup size for both roles");
    static_assert(bin_lds_words<NBMAX>() * 4 <= kBinEntries * 2 * sizeof(unsigned long long),
                  "the bin role's LDS fits the accumulate's image");
    __shared__ __attribute__((aligned(16))) unsigned long long acc[kBinEntries * 2];
    extern __shared__ uint32_t dyn[];
    __shared__ uint32_t s_tk;
    uint32_t* fw = retire + kFusedWords;  // ticket, finished, error, -, done[level]
    if constexpr (kFusedBwd == 2) {
        // the grid is one co-resident wave of workgroups (2 per CU): the
        // block index is the role (no ticket: one returning atomic per
        // workgroup on one word serialised ~1,550 of them, r07s)
        if (threadIdx.x == 0) s_tk = blockIdx.x;
    } else {
        if (threadIdx.x == 0) s_tk = atomicAdd(fw, 1u);
    }
    __syncthreads();
    const uint32_t tk = s_tk, nlev = bp.nlev;
    const uint32_t nbin = nlev * ycap, nextra = nred + next_batch.nlego;
    if (tk < nbin + nextra) {
        uint32_t bx, by;
        if (tk < nbin) {
            bx = tk % nlev;
            by = tk / nlev;
        } else if (tk < nbin + nred) {
            bx = nlev;  // the dW reduce column
            by = tk - nbin;
        } else {
            bx = nlev + (nred ? 1u : 0u);  // the sampler column
            by = tk - nbin - nred;
        }
        bin_block<D, NBMAX, true>(grad, inputs, offsets, grad_grid, B, L, lv, gridtype, align_corners, interp, im,
                                  bp, cursor, items, grad_layout, nonfinite, rj, nred, timing, next_batch, spill,
                                  spill_bad, nullptr, bx, by, ycap, reinterpret_cast<uint32_t*>(acc),
                                  ngp_reduce::DwProduct{});
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's stores and atomics have landed
        __syncthreads();
        if (threadIdx.x == 0) {
            if (tk == 0) atomicAdd(fw + 3, 1u);  // the timing entry is open (timing[0] stored atomically)
            if (tk < nbin) atomicAdd(fw + 4 + bx, 1u);
            // the last of the non-accumulate workgroups: every reader of this
            // batch's sample counter (the bin and sampler workgroups) is done
            if (atomicAdd(fw + 1, 1u) == nbin + nextra - 1 && reset_counter) {
                reset_counter[0] = 0;
                reset_counter[1] = 0;
            }
        }
        return;
    }
    const FusedSync fs{fw + 4, ycap, fw + 2, fw + 3};
    accum_block<true, true>(offsets, grad_grid, bp, cursor, retire, items, nonfinite, true, msums, marrive, timing,
                            nullptr, spill, spill_bad, wave_bins0, nimg, rows_in, wave_rows_max, tk - nbin - nextra,
                            nacc, acc, dyn, fs);
}

// GradScaler's inf/nan check over a grad range (levels the binned path does
// not cover): sets *flag.
__global__ void __launch_bounds__(256)
k_flag_nonfinite(const ngp_half* __restrict__ g, size_t n, int32_t* __restrict__ flag) {
    bool bad = false;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        bad |= !__builtin_isfinite((float)g[i]);
    if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(flag, 1);
}

// Host-side plan from a host copy of the offsets. Bins of hashed levels get
// twice their mean load (the hash spreads corners uniformly) + slack; bins of
// dense levels are z-slabs whose load follows the scene, so they get the
// worst case (every corner of every sample).
static BinPlan make_bin_plan(const int32_t* offsets_host, uint32_t L, uint32_t D, const GridLevels& lv,
                             bool align_corners, uint32_t B) {
    BinPlan bp{};
    const uint64_t items_all = (uint64_t)B << D;
    uint32_t bins = 0;
    uint64_t slots = 0;
    for (uint32_t l = 0; l < L; ++l) {
        const uint32_t hs = (uint32_t)(offsets_host[l + 1] - offsets_host[l]);
        const uint32_t nb = (hs + kBinEntries - 1) / kBinEntries;
        if (nb > kMaxBinsPerLevelBig || bins + nb > kMaxTotalBins) break;
        const double side = (double)(align_corners ? lv.res[l] : lv.res[l] + 1);
        const bool hashed = std::pow(side, (double)D) > (double)hs;
        if (!hashed && bp.img_bins == bins) bp.img_bins = bins + nb;  // still in the dense prefix
        const uint64_t cap = hashed ? std::min<uint64_t>(items_all, 2 * ((items_all + nb - 1) / nb) + 2048)
                                    : items_all;
        bp.nbins[l] = nb;
        bp.bin0[l] = bins;
        bp.cap[l] = (uint32_t)std::max<uint64_t>(cap, 1);
        bp.item0[l] = (uint32_t)slots;
        if (lv.res[l] <= kMergeMaxRes) bp.merge_mask |= 1ull << l;  // cells span several ray steps
        bp.mslot0[l] = bp.cap[l] > kSegItems ? bp.nmslots : kNoSlot;
        if (bp.cap[l] > kSegItems) bp.nmslots += nb;
        bins += nb;
        slots += (uint64_t)nb * bp.cap[l];
        bp.nlev = l + 1;
    }
    if (slots >= 0xffffffffull) bp.nlev = 0;  // item offsets are 32-bit: fall back to atomics
    for (uint32_t l = 0; l <= bp.nlev; ++l) bp.off[l] = (uint32_t)offsets_host[l];
    bp.total_bins = bins;
    bp.spill_entries = bp.nlev ? (uint32_t)offsets_host[bp.nlev] : 0u;
    return bp;
}

static size_t bin_counters_bytes(const BinPlan& bp) { return ((size_t)bp.total_bins * 4 + 255) / 256 * 256; }

// workspace: [bin cursors][retire counter][items][int64 sums of the multi-unit
// slots][their arrival counters][timing ring][spill image: int64 counts per
// binned table entry and channel][spill marks per bin]
static size_t bin_items_bytes(const BinPlan& bp) {
    size_t slots = 0;
    for (uint32_t l = 0; l < bp.nlev; ++l) slots += (size_t)bp.nbins[l] * bp.cap[l];
    return (slots * sizeof(BinItem) + 255) / 256 * 256;
}
static size_t bin_sums_offset(const BinPlan& bp) { return bin_counters_bytes(bp) + kRetireBytes + bin_items_bytes(bp); }
static size_t bin_arrive_offset(const BinPlan& bp) {
    return bin_sums_offset(bp) + (size_t)bp.nmslots * kBinEntries * 2 * sizeof(unsigned long long);
}
// the launch-timing ring (NGP_GRID_TIMING, include/ngp_hip.h): u32 words
static size_t bin_timing_offset(const BinPlan& bp) {
    return bin_arrive_offset(bp) + ((size_t)bp.nmslots * 4 + 255) / 256 * 256;
}
static size_t bin_spill_offset(const BinPlan& bp) {
    return bin_timing_offset(bp) + ((size_t)(kTimingEnds + NGP_GRID_TIMING_RING * NGP_GRID_TIMING_MAX_WG) * 4 + 255) /
                                       256 * 256;
}
static size_t bin_spill_bad_offset(const BinPlan& bp) {
    return bin_spill_offset(bp) + (size_t)bp.spill_entries * 2 * sizeof(unsigned long long);
}
static size_t bin_workspace_bytes(const BinPlan& bp) {
    return bin_spill_bad_offset(bp) + ((size_t)bp.total_bins * 4 + 255) / 256 * 256;
}

template <typename T, uint32_t D, uint32_t C>
__global__ void __launch_bounds__(256)
k_grid_input_bwd(const T* __restrict__ grad, const T* __restrict__ dy_dx,
                 T* __restrict__ grad_inputs, uint32_t B, uint32_t L, int32_t grad_layout) {
    using A = Acc<T>;
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= B * D) return;
    const uint32_t b = t / D;
    const uint32_t d = t - b * D;
    const T* dd = dy_dx + (size_t)b * L * D * C;
    typename A::S result = A::zero();
    for (uint32_t l = 0; l < L; l++) {
#pragma unroll
        for (uint32_t ch = 0; ch < C; ch++) {
            const size_t gi = grad_layout == 0 ? ((size_t)l * B + b) * C + ch
                                               : ((size_t)b * L + l) * C + ch;
            result = A::mac(result, A::load(grad + gi), A::load(dd + l * D * C + d * C + ch));
        }
    }
    grad_inputs[t] = result;
}

// TV gradient (reference gridencoder.cu:503-607). float / double only: the
// reference's half instantiation calls an empty at::Half atomicAdd stub
// (gridencoder.cu:22-26) and so never writes anything.
template <typename T, uint32_t D, uint32_t C>
__global__ void __launch_bounds__(256)
k_grid_tv(const T* __restrict__ inputs, const T* __restrict__ grid, T* __restrict__ grad,
          const int32_t* __restrict__ offsets, float weight, uint32_t B, uint32_t L, GridLevels lv,
          uint32_t gridtype, bool align_corners) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const uint32_t level = blockIdx.y;
    T x[D];
#pragma unroll
    for (uint32_t d = 0; d < D; d++) {
        x[d] = inputs[(size_t)b * D + d];
        if (x[d] < 0 || x[d] > 1) return;
    }
    const uint32_t off0 = (uint32_t)offsets[level];
    const uint32_t hs = (uint32_t)offsets[level + 1] - off0;
    const uint32_t hs_mask = (hs & (hs - 1)) == 0 ? hs - 1 : 0;
    const T* g = grid + (size_t)off0 * C;
    T* gr = grad + (size_t)off0 * C;
    const float scale = lv.scale[level];
    const uint32_t resolution = lv.res[level];
    uint32_t pg[D];
#pragma unroll
    for (uint32_t d = 0; d < D; d++) {
        float pos;
        if constexpr (sizeof(T) == 8) pos = (float)fma(x[d], (double)scale, align_corners ? 0.0 : 0.5);
        else pos = fmaf((float)x[d], scale, align_corners ? 0.0f : 0.5f);
        pg[d] = (uint32_t)floorf(pos);
    }
    T results[C], idelta[C];
#pragma unroll
    for (uint32_t c = 0; c < C; ++c) { results[c] = 0; idelta[c] = 0; }
    const uint32_t index = grid_index<D>(gridtype, align_corners, hs, hs_mask, resolution, pg) * C;
    const T w = (T)(weight / (2 * D));
#pragma unroll
    for (uint32_t d = 0; d < D; d++) {
        const uint32_t cur_d = pg[d];
        if (cur_d < resolution) {
            pg[d] = cur_d + 1;
            const uint32_t ir = grid_index<D>(gridtype, align_corners, hs, hs_mask, resolution, pg) * C;
#pragma unroll
            for (uint32_t c = 0; c < C; c++) {
                const T gv = g[index + c] - g[ir + c];
                results[c] += gv;
                idelta[c] = fma(gv, gv, idelta[c]);  // nvcc contracts the reference's += v * v
            }
        }
        if (cur_d > 0) {
            pg[d] = cur_d - 1;
            const uint32_t il = grid_index<D>(gridtype, align_corners, hs, hs_mask, resolution, pg) * C;
#pragma unroll
            for (uint32_t c = 0; c < C; c++) {
                const T gv = g[index + c] - g[il + c];
                results[c] += gv;
                idelta[c] = fma(gv, gv, idelta[c]);
            }
        }
        pg[d] = cur_d;
    }
#pragma unroll
    for (uint32_t c = 0; c < C; c++)
        atomicAdd(&gr[index + c], w * results[c] * (T)rsqrtf((float)(idelta[c] + (T)1e-9f)));
}

// ---- dispatch ---------------------------------------------------------------
template <typename T, typename E, uint32_t D>
int fwd_c(const float* inputs, const void* emb, const int32_t* offsets, void* out, uint32_t B,
          uint32_t C, uint32_t L, const GridLevels& lv, void* dy_dx, uint32_t gridtype,
          bool ac, uint32_t interp, int32_t layout, const InMap& im, hipStream_t st) {
    const dim3 grid(ngp_div_up(B, 256), L);
    const E* e = (const E*)emb;
    T* o = (T*)out;
    T* dd = (T*)dy_dx;
    if constexpr (std::is_same<T, ngp_half>::value && D == 3) {
        // large batches: the coarsest dense levels from LDS (k_grid_fwd_lds),
        // the pair kernel over the rest
        if (!dd && kFwdLdsLevels && B >= kFwdLdsMin && C == 2 && L > kFwdLdsLevels) {
            size_t ent = 0;
            for (uint32_t l = 0; l < kFwdLdsLevels; ++l) {  // a level holds at most its dense grid, 8-aligned
                const double side = ac ? lv.res[l] : lv.res[l] + 1.0;
                ent += ((size_t)(side * side * side) + 7) / 8 * 8;
            }
            if (ent * 4 <= 80 * 1024) {  // two workgroups per CU
                const uint32_t nb = std::min<uint32_t>(2 * ngp_num_cus(), ngp_div_up(B, 512));
                k_grid_fwd_lds<E, 3, (kFwdLdsLevels ? kFwdLdsLevels : 1u)><<<nb, 512, ent * 4, st>>>(
                    inputs, e, offsets, o, B, L, lv, gridtype, ac, interp, layout, im);
                const uint32_t Lr = L - kFwdLdsLevels;
                const uint32_t gpx = ((Lr + 7) / 8 + kFwdLevelsPerBlock - 1) / kFwdLevelsPerBlock;
                const dim3 gp(8 * gpx * ngp_div_up(B, 128));
                k_grid_fwd_pair<T, E, D, 2><<<gp, 256, 0, st>>>(inputs, e, offsets, o, B, L, lv, gridtype, ac, interp,
                                                                layout, im, kFwdLdsLevels);
                return ngp_check_launch("grid_encode_forward");
            }
        }
    }
    if (!dd && (sizeof(T) <= 4)) {
        // XCD-aware 1-D grid (see the kernel): 8 XCDs x level groups x point chunks
        const bool gm = B >= kFwdGroupMajorMin;
        const uint32_t kl = gm ? 1u : kFwdLevelsPerBlock;
        const uint32_t gpx = ((L + 7) / 8 + kl - 1) / kl;
        const dim3 gp(8 * (gpx * ngp_div_up(B, 128) + (!gm && L == 16 ? fwd_borrow_extra(B) : 0u)));
#define FWD_PAIR_CASE(CC)                                                                                     \
    (gm ? k_grid_fwd_pair<T, E, D, CC, 1><<<gp, 256, 0, st>>>(inputs, e, offsets, o, B, L, lv, gridtype, ac, \
                                                             interp, layout, im)                              \
        : k_grid_fwd_pair<T, E, D, CC><<<gp, 256, 0, st>>>(inputs, e, offsets, o, B, L, lv, gridtype, ac,     \
                                                          interp, layout, im))
        switch (C) {
            case 1: FWD_PAIR_CASE(1); break;
            case 2: FWD_PAIR_CASE(2); break;
            case 4: FWD_PAIR_CASE(4); break;
            case 8: FWD_PAIR_CASE(8); break;
            default: return ngp_set_error(NGP_ERR_UNSUPPORTED, "GridEncoding: C must be 1, 2, 4, or 8.");
        }
#undef FWD_PAIR_CASE
        return ngp_check_launch("grid_encode_forward");
    }
    switch (C) {
        case 1: k_grid_fwd<T, E, D, 1><<<grid, 256, 0, st>>>(inputs, e, offsets, o, B, L, lv, dd, gridtype, ac, interp, layout, im); break;
        case 2: k_grid_fwd<T, E, D, 2><<<grid, 256, 0, st>>>(inputs, e, offsets, o, B, L, lv, dd, gridtype, ac, interp, layout, im); break;
        case 4: k_grid_fwd<T, E, D, 4><<<grid, 256, 0, st>>>(inputs, e, offsets, o, B, L, lv, dd, gridtype, ac, interp, layout, im); break;
        case 8: k_grid_fwd<T, E, D, 8><<<grid, 256, 0, st>>>(inputs, e, offsets, o, B, L, lv, dd, gridtype, ac, interp, layout, im); break;
        default: return ngp_set_error(NGP_ERR_UNSUPPORTED, "GridEncoding: C must be 1, 2, 4, or 8.");
    }
    return ngp_check_launch("grid_encode_forward");
}

template <typename T, typename E = T>
int fwd_t(const float* inputs, const void* emb, const int32_t* offsets, void* out, uint32_t B,
          uint32_t D, uint32_t C, uint32_t L, const GridLevels& lv, void* dy_dx,
          uint32_t gridtype, bool ac, uint32_t interp, int32_t layout, hipStream_t st,
          const InMap& im = InMap{0.0f, 0.0f, nullptr}) {
    switch (D) {
        case 2: return fwd_c<T, E, 2>(inputs, emb, offsets, out, B, C, L, lv, dy_dx, gridtype, ac, interp, layout, im, st);
        case 3: return fwd_c<T, E, 3>(inputs, emb, offsets, out, B, C, L, lv, dy_dx, gridtype, ac, interp, layout, im, st);
        case 4: return fwd_c<T, E, 4>(inputs, emb, offsets, out, B, C, L, lv, dy_dx, gridtype, ac, interp, layout, im, st);
        case 5: return fwd_c<T, E, 5>(inputs, emb, offsets, out, B, C, L, lv, dy_dx, gridtype, ac, interp, layout, im, st);
        default: return ngp_set_error(NGP_ERR_UNSUPPORTED, "GridEncoding: D must be 2, 3, 4, or 5.");
    }
}

template <typename T, uint32_t D, uint32_t C>
int bwd_one(const void* grad, const float* inputs, const int32_t* offsets, void* gemb,
            uint32_t B, uint32_t L, const GridLevels& lv, const void* dy_dx, void* grad_inputs,
            uint32_t gridtype, bool ac, uint32_t interp, int32_t layout, hipStream_t st,
            const InMap& im) {
    const dim3 grid(ngp_div_up(B, 128), L);  // two lanes per point (corner pairs)
    k_grid_bwd<T, D, C><<<grid, 256, 0, st>>>((const T*)grad, inputs, offsets, (T*)gemb, B, L, lv,
                                               gridtype, ac, interp, layout, im, 0u);
    if (dy_dx && grad_inputs) {
        k_grid_input_bwd<T, D, C><<<ngp_div_up(B * D, 256), 256, 0, st>>>(
            (const T*)grad, (const T*)dy_dx, (T*)grad_inputs, B, L, layout);
    }
    return ngp_check_launch("grid_encode_backward");
}

template <typename T, uint32_t D>
int bwd_c(const void* grad, const float* inputs, const int32_t* offsets, void* gemb, uint32_t B,
          uint32_t C, uint32_t L, const GridLevels& lv, const void* dy_dx, void* gi,
          uint32_t gridtype, bool ac, uint32_t interp, int32_t layout, hipStream_t st,
          const InMap& im) {
    switch (C) {
        case 1: return bwd_one<T, D, 1>(grad, inputs, offsets, gemb, B, L, lv, dy_dx, gi, gridtype, ac, interp, layout, st, im);
        case 2: return bwd_one<T, D, 2>(grad, inputs, offsets, gemb, B, L, lv, dy_dx, gi, gridtype, ac, interp, layout, st, im);
        case 4: return bwd_one<T, D, 4>(grad, inputs, offsets, gemb, B, L, lv, dy_dx, gi, gridtype, ac, interp, layout, st, im);
        case 8: return bwd_one<T, D, 8>(grad, inputs, offsets, gemb, B, L, lv, dy_dx, gi, gridtype, ac, interp, layout, st, im);
        default: return ngp_set_error(NGP_ERR_UNSUPPORTED, "GridEncoding: C must be 1, 2, 4, or 8.");
    }
}

template <typename T>
int bwd_t(const void* grad, const float* inputs, const int32_t* offsets, void* gemb, uint32_t B,
          uint32_t D, uint32_t C, uint32_t L, const GridLevels& lv, const void* dy_dx, void* gi,
          uint32_t gridtype, bool ac, uint32_t interp, int32_t layout, hipStream_t st,
          const InMap& im = InMap{0.0f, 0.0f, nullptr}) {
    switch (D) {
        case 2: return bwd_c<T, 2>(grad, inputs, offsets, gemb, B, C, L, lv, dy_dx, gi, gridtype, ac, interp, layout, st, im);
        case 3: return bwd_c<T, 3>(grad, inputs, offsets, gemb, B, C, L, lv, dy_dx, gi, gridtype, ac, interp, layout, st, im);
        case 4: return bwd_c<T, 4>(grad, inputs, offsets, gemb, B, C, L, lv, dy_dx, gi, gridtype, ac, interp, layout, st, im);
        case 5: return bwd_c<T, 5>(grad, inputs, offsets, gemb, B, C, L, lv, dy_dx, gi, gridtype, ac, interp, layout, st, im);
        default: return ngp_set_error(NGP_ERR_UNSUPPORTED, "GridEncoding: D must be 2, 3, 4, or 5.");
    }
}

template <typename T, uint32_t D>
int tv_c(const void* inputs, const void* emb, void* grad, const int32_t* offsets, float weight,
         uint32_t B, uint32_t C, uint32_t L, const GridLevels& lv, uint32_t gridtype, bool ac,
         hipStream_t st) {
    const dim3 grid(ngp_div_up(B, 256), L);
    const T* in = (const T*)inputs;
    const T* e = (const T*)emb;
    T* g = (T*)grad;
    switch (C) {
        case 1: k_grid_tv<T, D, 1><<<grid, 256, 0, st>>>(in, e, g, offsets, weight, B, L, lv, gridtype, ac); break;
        case 2: k_grid_tv<T, D, 2><<<grid, 256, 0, st>>>(in, e, g, offsets, weight, B, L, lv, gridtype, ac); break;
        case 4: k_grid_tv<T, D, 4><<<grid, 256, 0, st>>>(in, e, g, offsets, weight, B, L, lv, gridtype, ac); break;
        case 8: k_grid_tv<T, D, 8><<<grid, 256, 0, st>>>(in, e, g, offsets, weight, B, L, lv, gridtype, ac); break;
        default: return ngp_set_error(NGP_ERR_UNSUPPORTED, "GridEncoding: C must be 1, 2, 4, or 8.");
    }
    return ngp_check_launch("grad_total_variation");
}

template <typename T>
int tv_t(const void* inputs, const void* emb, void* grad, const int32_t* offsets, float weight,
         uint32_t B, uint32_t D, uint32_t C, uint32_t L, const GridLevels& lv, uint32_t gridtype,
         bool ac, hipStream_t st) {
    switch (D) {
        case 2: return tv_c<T, 2>(inputs, emb, grad, offsets, weight, B, C, L, lv, gridtype, ac, st);
        case 3: return tv_c<T, 3>(inputs, emb, grad, offsets, weight, B, C, L, lv, gridtype, ac, st);
        case 4: return tv_c<T, 4>(inputs, emb, grad, offsets, weight, B, C, L, lv, gridtype, ac, st);
        case 5: return tv_c<T, 5>(inputs, emb, grad, offsets, weight, B, C, L, lv, gridtype, ac, st);
        default: return ngp_set_error(NGP_ERR_UNSUPPORTED, "GridEncoding: D must be 2, 3, 4, or 5.");
    }
}

int check_common(uint32_t L, const void* a, const void* b, const void* c) {
    NGP_REQUIRE(L >= 1 && L <= kMaxLevels, NGP_ERR_ARG, "GridEncoding: L must be in [1, %u], got %u", kMaxLevels, L);
    NGP_REQUIRE(a && b && c, NGP_ERR_ARG, "GridEncoding: null tensor pointer");
    return NGP_OK;
}

}  // namespace

extern "C" int ngp_grid_encode_forward(const float* inputs, const void* embeddings,
                                       const int32_t* offsets, void* outputs, uint32_t B,
                                       uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H,
                                       void* dy_dx, uint32_t gridtype, int32_t align_corners,
                                       uint32_t interp, int32_t dtype, int32_t out_layout,
                                       void* stream) {
    if (int e = check_common(L, embeddings, offsets, outputs)) return e;
    if (B == 0) return NGP_OK;
    NGP_REQUIRE(inputs, NGP_ERR_ARG, "GridEncoding: null inputs");
    GridLevels lv;
    make_levels(lv, L, S, H);
    const bool ac = align_corners != 0;
    hipStream_t st = ngp_stream(stream);
    switch (dtype) {
        case NGP_DTYPE_F32: return fwd_t<float>(inputs, embeddings, offsets, outputs, B, D, C, L, lv, dy_dx, gridtype, ac, interp, out_layout, st);
        case NGP_DTYPE_F16: return fwd_t<ngp_half>(inputs, embeddings, offsets, outputs, B, D, C, L, lv, dy_dx, gridtype, ac, interp, out_layout, st);
        case NGP_DTYPE_F64: return fwd_t<double>(inputs, embeddings, offsets, outputs, B, D, C, L, lv, dy_dx, gridtype, ac, interp, out_layout, st);
        default: return ngp_set_error(NGP_ERR_ARG, "embeddings must be a floating tensor");
    }
}

extern "C" int ngp_grid_encode_backward(const void* grad, const float* inputs,
                                        const void* embeddings, const int32_t* offsets,
                                        void* grad_embeddings, uint32_t B, uint32_t D, uint32_t C,
                                        uint32_t L, float S, uint32_t H, const void* dy_dx,
                                        void* grad_inputs, uint32_t gridtype,
                                        int32_t align_corners, uint32_t interp, int32_t dtype,
                                        int32_t grad_layout, void* stream) {
    (void)embeddings;
    if (int e = check_common(L, grad, offsets, grad_embeddings)) return e;
    if (B == 0) return NGP_OK;
    NGP_REQUIRE(inputs, NGP_ERR_ARG, "GridEncoding: null inputs");
    GridLevels lv;
    make_levels(lv, L, S, H);
    const bool ac = align_corners != 0;
    hipStream_t st = ngp_stream(stream);
    switch (dtype) {
        case NGP_DTYPE_F32: return bwd_t<float>(grad, inputs, offsets, grad_embeddings, B, D, C, L, lv, dy_dx, grad_inputs, gridtype, ac, interp, grad_layout, st);
        case NGP_DTYPE_F16: return bwd_t<ngp_half>(grad, inputs, offsets, grad_embeddings, B, D, C, L, lv, dy_dx, grad_inputs, gridtype, ac, interp, grad_layout, st);
        case NGP_DTYPE_F64: return bwd_t<double>(grad, inputs, offsets, grad_embeddings, B, D, C, L, lv, dy_dx, grad_inputs, gridtype, ac, interp, grad_layout, st);
        default: return ngp_set_error(NGP_ERR_ARG, "grad must be a floating tensor");
    }
}

extern "C" int ngp_grad_total_variation(const void* inputs, const void* embeddings, void* grad,
                                        const int32_t* offsets, float weight, uint32_t B,
                                        uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H,
                                        uint32_t gridtype, int32_t align_corners, int32_t dtype,
                                        void* stream) {
    if (int e = check_common(L, embeddings, offsets, grad)) return e;
    if (B == 0) return NGP_OK;
    GridLevels lv;
    make_levels(lv, L, S, H);
    const bool ac = align_corners != 0;
    hipStream_t st = ngp_stream(stream);
    switch (dtype) {
        case NGP_DTYPE_F32: return tv_t<float>(inputs, embeddings, grad, offsets, weight, B, D, C, L, lv, gridtype, ac, st);
        case NGP_DTYPE_F64: return tv_t<double>(inputs, embeddings, grad, offsets, weight, B, D, C, L, lv, gridtype, ac, st);
        case NGP_DTYPE_F16:
            return ngp_set_error(NGP_ERR_UNSUPPORTED, "grad_total_variation: half embeddings are not supported (call it outside autocast, as GridEncoder.grad_total_variation does)");
        default: return ngp_set_error(NGP_ERR_ARG, "embeddings must be a floating tensor");
    }
}

/* Fused train-step entry points (DESIGN.md "fused step"): world-space inputs
 * normalised in-kernel exactly as GridEncoder.forward does, an fp32 table
 * read as half (the reference's embeddings.half()), fp16 [B, L*C] outputs /
 * output grads, fp16 grad table, rows clipped at *count. */
extern "C" int ngp_grid_encode_forward_fused(const float* xyz, float bound, const void* embeddings,
                                             int32_t emb_dtype, const int32_t* offsets, void* outputs,
                                             uint32_t B,
                                             const int32_t* count, uint32_t D, uint32_t C, uint32_t L,
                                             float S, uint32_t H, uint32_t gridtype,
                                             int32_t align_corners, uint32_t interp, int32_t out_layout,
                                             void* stream) {
    if (int e = check_common(L, embeddings, offsets, outputs)) return e;
    NGP_REQUIRE(xyz && bound > 0.0f, NGP_ERR_ARG, "grid_encode_forward_fused: null xyz or bound <= 0");
    if (B == 0) return NGP_OK;
    GridLevels lv;
    make_levels(lv, L, S, H);
    const InMap im{bound, 1.0f / (2.0f * bound), count};
    NGP_REQUIRE(emb_dtype == NGP_DTYPE_F32 || emb_dtype == NGP_DTYPE_F16, NGP_ERR_ARG,
                "grid_encode_forward_fused: emb_dtype %d (F32 or F16)", emb_dtype);
    if (emb_dtype == NGP_DTYPE_F16)
        return fwd_t<ngp_half, ngp_half>(xyz, embeddings, offsets, outputs, B, D, C, L, lv, nullptr, gridtype,
                                         align_corners != 0, interp, out_layout, ngp_stream(stream), im);
    return fwd_t<ngp_half, float>(xyz, embeddings, offsets, outputs, B, D, C, L, lv, nullptr, gridtype,
                                  align_corners != 0, interp, out_layout, ngp_stream(stream), im);
}

extern "C" int ngp_grid_encode_forward_fused_tail(const float* xyz, float bound, const void* embeddings,
                                                  int32_t emb_dtype, const int32_t* offsets, void* outputs, uint32_t B,
                                                  const int32_t* count, uint32_t D, uint32_t C, uint32_t L, float S,
                                                  uint32_t H, uint32_t gridtype, int32_t align_corners,
                                                  uint32_t interp, void* state, float growth_factor,
                                                  float backoff_factor, int32_t growth_interval,
                                                  int32_t scaler_enabled, const float* loss_ray, uint32_t n_rays,
                                                  int32_t n_nets, const void* const* mlp_weights,
                                                  const uint32_t* in_dims, const uint32_t* hidden_dims,
                                                  const uint32_t* num_layers, void* const* images, void* stream) {
    if (int e = check_common(L, embeddings, offsets, outputs)) return e;
    NGP_REQUIRE(xyz && bound > 0.0f, NGP_ERR_ARG, "grid_encode_forward_fused_tail: null xyz or bound <= 0");
    NGP_REQUIRE(D == 3 && C == 2, NGP_ERR_UNSUPPORTED, "grid_encode_forward_fused_tail: D 3, C 2 only");
    NGP_REQUIRE(emb_dtype == NGP_DTYPE_F32 || emb_dtype == NGP_DTYPE_F16, NGP_ERR_ARG,
                "grid_encode_forward_fused_tail: emb_dtype %d (F32 or F16)", emb_dtype);
    NGP_REQUIRE(!state || loss_ray, NGP_ERR_ARG, "grid_encode_forward_fused_tail: the bookkeeping needs loss_ray");
    FwdTail ft{};
    if (state) {
        ft.end = static_cast<ngp_step::StepState*>(state);
        ft.sa = ngp_step::ScalerArgs{growth_factor, backoff_factor, growth_interval, scaler_enabled,
                                     n_rays ? 1.0f / (float)n_rays : 0.0f};
        ft.loss_ray = loss_ray;
        ft.n_rays = n_rays;
    }
    if (n_nets > 0)
        if (int e = ngp_pack::build_jobs(n_nets, mlp_weights, in_dims, hidden_dims, num_layers, images, ft.jobs))
            return e;
    GridLevels lv;
    make_levels(lv, L, S, H);
    const InMap im{bound, 1.0f / (2.0f * bound), count};
    const bool ac = align_corners != 0;
    const bool gm = B >= kFwdGroupMajorMin;
    const uint32_t kl = gm ? 1u : kFwdLevelsPerBlock;
    const uint32_t nfwd = B ? 8u * ((((L + 7) / 8 + kl - 1) / kl) * ngp_div_up(B, 128) +
                                    (!gm && L == 16 ? fwd_borrow_extra(B) : 0u))
                            : 0u;
    const dim3 grid(nfwd + (ft.end ? 1u : 0u) + (uint32_t)ft.jobs.n);
    if (grid.x == 0) return NGP_OK;
    hipStream_t st = ngp_stream(stream);
    ngp_half* o = static_cast<ngp_half*>(outputs);
#define FWD_TAIL_LAUNCH(E_)                                                                                          \
    (gm ? k_grid_fwd_tail<ngp_half, E_, 3, 2, 1><<<grid, 256, 0, st>>>(xyz, static_cast<const E_*>(embeddings),   \
                                                                        offsets, o, B, L, lv, gridtype, ac, interp, \
                                                                        0, im, ft)                                  \
        : k_grid_fwd_tail<ngp_half, E_, 3, 2><<<grid, 256, 0, st>>>(xyz, static_cast<const E_*>(embeddings), offsets, \
                                                                     o, B, L, lv, gridtype, ac, interp, 0, im, ft))
    if (emb_dtype == NGP_DTYPE_F16)
        FWD_TAIL_LAUNCH(ngp_half);
    else
        FWD_TAIL_LAUNCH(float);
#undef FWD_TAIL_LAUNCH
    return ngp_check_launch("grid_encode_forward_fused_tail");
}

extern "C" size_t ngp_grid_encode_backward_fused_workspace_bytes(uint32_t B, uint32_t D, uint32_t C,
                                                                uint32_t L, float S, uint32_t H,
                                                                int32_t align_corners,
                                                                const int32_t* offsets_host) {
    if (!offsets_host || C != 2 || D < 2 || D > 5 || L == 0 || L > kMaxLevels) return 0;
    GridLevels lv;
    make_levels(lv, L, S, H);
    const BinPlan bp = make_bin_plan(offsets_host, L, D, lv, align_corners != 0, B);
    return bp.nlev ? bin_workspace_bytes(bp) : 0;
}

extern "C" size_t ngp_grid_encode_backward_fused_counter_bytes(uint32_t B, uint32_t D, uint32_t C, uint32_t L,
                                                               float S, uint32_t H, int32_t align_corners,
                                                               const int32_t* offsets_host) {
    if (!offsets_host || C != 2 || D < 2 || D > 5 || L == 0 || L > kMaxLevels) return 0;
    GridLevels lv;
    make_levels(lv, L, S, H);
    const BinPlan bp = make_bin_plan(offsets_host, L, D, lv, align_corners != 0, B);
    return bp.nlev ? bin_counters_bytes(bp) + kRetireBytes : 0;
}

namespace {
__global__ void __launch_bounds__(256)
k_lego_draw(BinLego bl) {
    ngp_head::lego_rays_block(blockIdx.x, bl.nlego, bl.poses, bl.sc, bl.N, bl.st, bl.out);
}

int bwd_fused_impl(const void* grad, const float* xyz, float bound, const int32_t* offsets, void* grad_embeddings,
                   uint32_t B, const int32_t* count, uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H,
                   uint32_t gridtype, int32_t align_corners, uint32_t interp, const int32_t* offsets_host,
                   void* workspace, size_t workspace_bytes, int32_t grad_layout, int32_t* nonfinite,
                   void* stream, const ngp_reduce::ReduceJobs* rj = nullptr,
                   uint32_t nred = 0, const BinLego* blp = nullptr, const int32_t* rows = nullptr,
                   const ngp_reduce::DwProduct* dwp = nullptr) {
    if (int e = check_common(L, grad, offsets, grad_embeddings)) return e;
    const bool zeroed = (grad_layout & NGP_GRID_GRAD_ZEROED) != 0;
    const bool external = (grad_layout & NGP_GRID_CURSORS_EXTERNAL) != 0;
    const bool timed = (grad_layout & NGP_GRID_TIMING) != 0;
    grad_layout &= ~(NGP_GRID_GRAD_ZEROED | NGP_GRID_CURSORS_EXTERNAL | NGP_GRID_TIMING);
    NGP_REQUIRE(grad_layout == 0 || grad_layout == 1, NGP_ERR_ARG,
                "grid_encode_backward_fused: grad_layout 0 ([L,B,C]) or 1 ([B,L*C])");
    NGP_REQUIRE(xyz && bound > 0.0f, NGP_ERR_ARG, "grid_encode_backward_fused: null xyz or bound <= 0");
    NGP_REQUIRE(!nonfinite || offsets_host, NGP_ERR_ARG,
                "grid_encode_backward_fused: the nonfinite check needs offsets_host");
    if (B == 0) return NGP_OK;
    GridLevels lv;
    make_levels(lv, L, S, H);
    InMap im{bound, 1.0f / (2.0f * bound), count};
    im.rows = rows;
    hipStream_t st = ngp_stream(stream);
    const bool ac = align_corners != 0;
    BinPlan bp{};
    if (workspace && offsets_host && C == 2 && D == 3) {
        bp = make_bin_plan(offsets_host, L, D, lv, ac, B);
        if (bp.nlev)
            NGP_REQUIRE(workspace_bytes >= bin_workspace_bytes(bp), NGP_ERR_ARG,
                        "grid_encode_backward_fused: workspace of %zu bytes required, got %zu",
                        bin_workspace_bytes(bp), workspace_bytes);
    }
    if (bp.nlev) {  // the workspace's counters start zeroed and are left zeroed
        uint32_t* cursor = static_cast<uint32_t*>(workspace);
        uint32_t* retire = reinterpret_cast<uint32_t*>(static_cast<char*>(workspace) + bin_counters_bytes(bp));
        BinItem* items = reinterpret_cast<BinItem*>(static_cast<char*>(workspace) + bin_counters_bytes(bp) + kRetireBytes);
        unsigned long long* msums =
            reinterpret_cast<unsigned long long*>(static_cast<char*>(workspace) + bin_sums_offset(bp));
        uint32_t* timing =
            timed ? reinterpret_cast<uint32_t*>(static_cast<char*>(workspace) + bin_timing_offset(bp)) : nullptr;
        uint32_t* marrive = reinterpret_cast<uint32_t*>(static_cast<char*>(workspace) + bin_arrive_offset(bp));
        auto* spill = reinterpret_cast<unsigned long long*>(static_cast<char*>(workspace) + bin_spill_offset(bp));
        auto* spill_bad = reinterpret_cast<uint32_t*>(static_cast<char*>(workspace) + bin_spill_bad_offset(bp));
        // (level, point block) + one column of slab-reduce blocks when merged
        const ngp_reduce::ReduceJobs rjv = rj ? *rj : ngp_reduce::ReduceJobs{};
        if (!rj) nred = 0;
        // + one column of the next batch's sampler blocks (blp, fully binned plans only)
        const BinLego bl = blp && bp.nlev == L ? *blp : BinLego{};
        // the dW product job rides in the reduce column (its tiles: fewer than the reduce's blocks)
        const ngp_reduce::DwProduct dw = dwp && nred ? *dwp : ngp_reduce::DwProduct{};
        NGP_REQUIRE(dw.blocks <= nred, NGP_ERR_ARG, "grid_encode_backward_fused: %u dW tiles for %u reduce blocks",
                    dw.blocks, nred);
        const dim3 grid(bp.nlev + (nred ? 1u : 0u) + (bl.nlego ? 1u : 0u),
                        std::max(std::max(std::min(ngp_div_up(B, kBinPts), kBinYCap), nred), bl.nlego));
        uint32_t nbmax = 0;
        for (uint32_t l = 0; l < bp.nlev; ++l) nbmax = std::max(nbmax, bp.nbins[l]);
        // the one-launch form (k_grid_bwd_fused) where the wave bins run: the
        // same kernels' work, the accumulate's waits per level
        const bool waves_cfg = zeroed && external && kWaveBins && bp.img_bins < bp.total_bins;
        const bool fused_fits = kFusedBwd != 2 ||
                                bp.nlev * std::min(ngp_div_up(B, kBinPts), 8u) + nred + bl.nlego + kAccImageWgs + 64 <=
                                    2 * ngp_num_cus();
        if (kFusedBwd && waves_cfg && fused_fits && B >= 1 && !dw.blocks) {
            const uint32_t img_bins = bp.img_bins;
            auto two_fit = [](size_t d) { return 2 * (d + kAccStaticLds) <= 160 * 1024; };
            const size_t dyn_all = (2 * (size_t)bp.total_bins + 1) * sizeof(uint32_t);
            const bool dense_ok = two_fit(dyn_all);
            const size_t dyn = dense_ok ? dyn_all : (2 * (size_t)img_bins + 1) * sizeof(uint32_t);
            const uint32_t per_cu = two_fit(dyn) ? 2u : 1u;
            const uint32_t nacc = per_cu * ngp_num_cus();
            const uint32_t nimg = img_bins ? std::min(kAccImageWgs, nacc / 2) : 0u;
            uint32_t wave_rows_max = 0xffffffffu;
            if (dense_ok) {
                uint32_t hl = 0;
                while (hl + 1 < bp.nlev && bp.bin0[hl + 1] <= img_bins) ++hl;
                wave_rows_max = (uint32_t)std::min<uint64_t>(0xfffffffeu, (uint64_t)kWaveMax * bp.nbins[hl] >> 3);
            }
            const uint32_t ycap = std::min(ngp_div_up(B, kBinPts), kFusedBwd == 2 ? 8u : kFusedYCap);
            uint32_t nacc_l = nacc;
            if (kFusedBwd == 2) {  // one co-resident grid: the accumulate takes what the bin roles leave
                const uint32_t used = bp.nlev * ycap + nred + bl.nlego;
                nacc_l = used + nimg + 64 <= nacc ? nacc - used : 0u;
            }
            const uint32_t nblocks = bp.nlev * ycap + nred + bl.nlego + nacc_l;
            int32_t* reset = bl.nlego ? bl.out.counter : nullptr;
            const uint32_t* rows_in = reinterpret_cast<const uint32_t*>(count);
            if (nbmax <= kMaxBinsPerLevel)
                k_grid_bwd_fused<3, kMaxBinsPerLevel><<<nblocks, kAccThreads, dyn, st>>>(
                    (const ngp_half*)grad, xyz, offsets, (ngp_half*)grad_embeddings, B, L, lv, gridtype, ac, interp,
                    im, bp, cursor, items, grad_layout, nonfinite, rjv, nred, timing, bl, spill, spill_bad, retire,
                    msums, marrive, reset, img_bins, nimg, rows_in, wave_rows_max, ycap, nacc_l);
            else
                k_grid_bwd_fused<3, kMaxBinsPerLevelBig><<<nblocks, kAccThreads, dyn, st>>>(
                    (const ngp_half*)grad, xyz, offsets, (ngp_half*)grad_embeddings, B, L, lv, gridtype, ac, interp,
                    im, bp, cursor, items, grad_layout, nonfinite, rjv, nred, timing, bl, spill, spill_bad, retire,
                    msums, marrive, reset, img_bins, nimg, rows_in, wave_rows_max, ycap, nacc_l);
        } else {
            if (nbmax <= kMaxBinsPerLevel)
                k_grid_bwd_bin<3, kMaxBinsPerLevel><<<grid, kBinPts, bin_lds_words<kMaxBinsPerLevel>() * 4, st>>>(
                    (const ngp_half*)grad, xyz, offsets, (ngp_half*)grad_embeddings, B, L, lv, gridtype, ac, interp,
                    im, bp, cursor, items, grad_layout, nonfinite, rjv, nred, timing, bl, spill, spill_bad, retire + kRowsWord,
                    dw);
            else
                k_grid_bwd_bin<3, kMaxBinsPerLevelBig><<<grid, kBinPts, bin_lds_words<kMaxBinsPerLevelBig>() * 4, st>>>(
                    (const ngp_half*)grad, xyz, offsets, (ngp_half*)grad_embeddings, B, L, lv, gridtype, ac, interp,
                    im, bp, cursor, items, grad_layout, nonfinite, rjv, nred, timing, bl, spill, spill_bad, retire + kRowsWord,
                    dw);
            // the hashed levels' bins one per wave (wave_bin) when the grad is
            // cleared and the caller clears the cursors (the fused step): the
            // image path then covers only the dense levels' bins, on the first
            // kAccImageWgs workgroups
            const bool waves = zeroed && external && kWaveBins && bp.img_bins < bp.total_bins;
            const uint32_t img_bins = waves ? bp.img_bins : bp.total_bins;
            // two persistent workgroups per CU while both fit the CU's LDS (the
            // 64 KiB image + two words per bin), else one. With the wave bins the
            // image path may take every bin in the dense regime (more rows than
            // wave_rows_max: ~kWaveMax items per hashed bin), when two workgroups
            // per CU still fit that; else the wave bins take the hashed levels
            // whatever the rows.
            auto two_fit = [](size_t d) { return 2 * (d + kAccStaticLds) <= 160 * 1024; };
            const size_t dyn_all = (2 * (size_t)bp.total_bins + 1) * sizeof(uint32_t);
            const bool dense_ok = waves && two_fit(dyn_all);
            const size_t dyn = dense_ok || !waves ? dyn_all : (2 * (size_t)img_bins + 1) * sizeof(uint32_t);
            const uint32_t per_cu = two_fit(dyn) ? 2u : 1u;
            const uint32_t grid_acc = per_cu * ngp_num_cus();
            const uint32_t nimg = waves ? (img_bins ? std::min(kAccImageWgs, grid_acc / 2) : 0u) : grid_acc;
            uint32_t wave_rows_max = 0xffffffffu;
            if (dense_ok) {
                uint32_t hl = 0;  // the first level of the wave bins
                while (hl + 1 < bp.nlev && bp.bin0[hl + 1] <= img_bins) ++hl;
                wave_rows_max = (uint32_t)std::min<uint64_t>(0xfffffffeu, (uint64_t)kWaveMax * bp.nbins[hl] >> 3);
            }
            uint32_t* rows_word = retire + kRowsWord;  // written by the bin launch
            int32_t* reset = bl.nlego ? bl.out.counter : nullptr;
            if (zeroed)
                k_grid_bin_accum<true><<<grid_acc, kAccThreads, dyn, st>>>(
                    offsets, (ngp_half*)grad_embeddings, bp, cursor, retire, items, nonfinite, external, msums,
                    marrive, timing, reset, spill, spill_bad, img_bins, nimg, waves ? rows_word : nullptr, wave_rows_max);
            else
                k_grid_bin_accum<false><<<grid_acc, kAccThreads, dyn, st>>>(
                    offsets, (ngp_half*)grad_embeddings, bp, cursor, retire, items, nonfinite, external, msums,
                    marrive, timing, reset, spill, spill_bad, img_bins, nimg, waves ? rows_word : nullptr, wave_rows_max);
        }
    }
    if (bp.nlev < L) {  // levels past the binned prefix: merged atomics
        if (D == 3 && C == 2) {
            const dim3 grid(ngp_div_up(B, 128), L - bp.nlev);
            k_grid_bwd<ngp_half, 3, 2><<<grid, 256, 0, st>>>((const ngp_half*)grad, xyz, offsets,
                (ngp_half*)grad_embeddings, B, L, lv, gridtype, ac, interp, grad_layout, im, bp.nlev);
        } else {
            if (int e = bwd_t<ngp_half>(grad, xyz, offsets, grad_embeddings, B, D, C, L, lv, nullptr, nullptr,
                                        gridtype, ac, interp, grad_layout, st, im))
                return e;
        }
        if (nonfinite) {  // those levels' atomics are not checked: scan their grads
            const size_t e0 = (size_t)offsets_host[bp.nlev] * C, e1 = (size_t)offsets_host[L] * C;
            const uint32_t blocks = (uint32_t)std::min<size_t>(ngp_div_up(e1 - e0, 256), 4096);
            k_flag_nonfinite<<<blocks, 256, 0, st>>>((const ngp_half*)grad_embeddings + e0, e1 - e0, nonfinite);
        }
    }
    if (blp && !(bp.nlev && bp.nlev == L)) {  // not carried by a bin launch: the draw after the backward
        BinLego b2 = *blp;
        b2.out.keep_counter = 0;
        b2.nlego = ngp_div_up(b2.N, 256);
        k_lego_draw<<<b2.nlego, 256, 0, st>>>(b2);
    }
    return ngp_check_launch("grid_encode_backward_fused");
}
}  // namespace

extern "C" size_t ngp_grid_encode_backward_fused_timing_offset(uint32_t B, uint32_t D, uint32_t C, uint32_t L,
                                                               float S, uint32_t H, int32_t align_corners,
                                                               const int32_t* offsets_host) {
    if (!offsets_host || C != 2 || D != 3 || L == 0 || L > kMaxLevels) return 0;
    GridLevels lv;
    make_levels(lv, L, S, H);
    const BinPlan bp = make_bin_plan(offsets_host, L, D, lv, align_corners != 0, B);
    return bp.nlev ? bin_timing_offset(bp) : 0;
}

extern "C" int ngp_grid_encode_backward_fused(const void* grad, const float* xyz, float bound,
                                              const int32_t* offsets, void* grad_embeddings,
                                              uint32_t B, const int32_t* count, uint32_t D,
                                              uint32_t C, uint32_t L, float S, uint32_t H,
                                              uint32_t gridtype, int32_t align_corners,
                                              uint32_t interp, const int32_t* offsets_host,
                                              void* workspace, size_t workspace_bytes, int32_t grad_layout,
                                              int32_t* nonfinite, void* stream) {
    return bwd_fused_impl(grad, xyz, bound, offsets, grad_embeddings, B, count, D, C, L, S, H, gridtype,
                          align_corners, interp, offsets_host, workspace, workspace_bytes, grad_layout, nonfinite,
                          stream);
}

extern "C" int ngp_grid_encode_backward_fused_reduce(const void* grad, const float* xyz, float bound,
                                                     const int32_t* offsets, void* grad_embeddings, uint32_t B,
                                                     const int32_t* count, uint32_t D, uint32_t C, uint32_t L,
                                                     float S, uint32_t H, uint32_t gridtype,
                                                     int32_t align_corners, uint32_t interp,
                                                     const int32_t* offsets_host, void* workspace,
                                                     size_t workspace_bytes, int32_t grad_layout,
                                                     int32_t* nonfinite, int32_t n_nets,
                                                     void* const* mlp_workspaces, const uint32_t* mlp_Bs,
                                                     const uint32_t* in_dims, const uint32_t* hidden_dims,
                                                     const uint32_t* num_layers, void* const* grad_weights,
                                                     int32_t* mlp_nonfinite, void* stream) {
    NGP_REQUIRE(n_nets >= 1 && n_nets <= ngp_reduce::kMaxReduceJobs && mlp_workspaces && mlp_Bs && in_dims &&
                    hidden_dims && num_layers && grad_weights,
                NGP_ERR_ARG, "grid_encode_backward_fused_reduce: 1..%d networks with their arguments",
                ngp_reduce::kMaxReduceJobs);
    // the plan decides whether there is a bin launch to carry the reduce
    bool binned = false;
    if (workspace && offsets_host && C == 2 && D == 3 && L >= 1 && L <= kMaxLevels) {
        GridLevels lv;
        make_levels(lv, L, S, H);
        binned = make_bin_plan(offsets_host, L, D, lv, align_corners != 0, B).nlev > 0;
    }
    if (!binned) {  // no bin launch: the reduce on its own, then the backward
        if (int e = ngp_ffmlp_reduce(n_nets, mlp_workspaces, mlp_Bs, in_dims, hidden_dims, num_layers, grad_weights,
                                     NGP_DTYPE_F16, mlp_nonfinite, stream))
            return e;
        return ngp_grid_encode_backward_fused(grad, xyz, bound, offsets, grad_embeddings, B, count, D, C, L, S, H,
                                              gridtype, align_corners, interp, offsets_host, workspace,
                                              workspace_bytes, grad_layout, nonfinite, stream);
    }
    ngp_reduce::ReduceJobs rj{};
    const uint32_t nred = ngp_reduce::build_reduce_jobs(n_nets, mlp_workspaces, mlp_Bs, in_dims, hidden_dims,
                                                        num_layers, grad_weights, mlp_nonfinite, rj);
    return bwd_fused_impl(grad, xyz, bound, offsets, grad_embeddings, B, count, D, C, L, S, H, gridtype,
                          align_corners, interp, offsets_host, workspace, workspace_bytes, grad_layout, nonfinite,
                          stream, &rj, nred);
}

static int reduce_batch_impl(
    const void* grad, const float* xyz, float bound, const int32_t* offsets, void* grad_embeddings, uint32_t B,
    const int32_t* count, uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H, uint32_t gridtype,
    int32_t align_corners, uint32_t interp, const int32_t* offsets_host, void* workspace, size_t workspace_bytes,
    int32_t grad_layout, int32_t* nonfinite, int32_t n_nets, void* const* mlp_workspaces, const uint32_t* mlp_Bs,
    const uint32_t* in_dims, const uint32_t* hidden_dims, const uint32_t* num_layers, void* const* grad_weights,
    int32_t* mlp_nonfinite, const ngp_batch_job* job, void* stream, const int32_t* rows,
    const ngp_image_source* src = nullptr, const void* dw_stash = nullptr, uint32_t dw_stash_rows = 0,
    uint32_t dw_rows_max = 0) {
    NGP_REQUIRE(job && job->state && job->counter && job->poses && job->N > 0 && job->n_poses > 0, NGP_ERR_ARG,
                "grid_encode_backward_fused_reduce_batch: incomplete batch job");
    NGP_REQUIRE(job->nboxes >= 0 && job->nboxes <= ngp_head::kMaxBoxes, NGP_ERR_ARG,
                "grid_encode_backward_fused_reduce_batch: at most %d boxes", ngp_head::kMaxBoxes);
    NGP_REQUIRE(n_nets >= 1 && n_nets <= ngp_reduce::kMaxReduceJobs && mlp_workspaces && mlp_Bs && in_dims &&
                    hidden_dims && num_layers && grad_weights,
                NGP_ERR_ARG, "grid_encode_backward_fused_reduce_batch: 1..%d networks with their arguments",
                ngp_reduce::kMaxReduceJobs);
    BinLego bl{};
    bl.sc = ngp_head::make_scene(job->n_poses, job->intrinsics4, job->H, job->W, job->boxes, job->nboxes,
                                 job->aabb6, job->min_near, job->seed);
    bl.out = ngp_head::LegoOut{job->rays_o, job->rays_d, job->rgba, job->bg, job->nears, job->fars, job->noises,
                               job->counter, job->step_counter, 1};
    if (src) ngp_head::set_image_source(bl.sc, bl.out, src);  // (checked by the caller)
    bl.poses = job->poses;
    bl.st = static_cast<ngp_step::StepState*>(job->state);
    bl.N = job->N;
    bl.nlego = ngp_div_up(job->N, kBinPts);
    ngp_reduce::ReduceJobs rj{};
    const uint32_t nred = ngp_reduce::build_reduce_jobs(n_nets, mlp_workspaces, mlp_Bs, in_dims, hidden_dims,
                                                        num_layers, grad_weights, mlp_nonfinite, rj);
    if (rows) rj.live = count;  // the slabs of ngp_nerf_backward_live over the same live rows
    // the stash of ngp_nerf_backward_live_dw: the product column (or its own launch where nothing is binned)
    ngp_reduce::DwProduct dw{};
    if (dw_stash) {
        NGP_REQUIRE(rows && n_nets == 2, NGP_ERR_ARG,
                    "grid_encode_backward_fused_dw_batch: a row list and the sigma and colour networks");
        if (int e = ngp_reduce::build_dw_product(mlp_Bs, in_dims, hidden_dims, num_layers, grad_weights,
                                                 mlp_nonfinite, count, dw_stash, dw_stash_rows, dw_rows_max, dw))
            return e;
    }
    bool binned = false;
    if (workspace && offsets_host && C == 2 && D == 3 && L >= 1 && L <= kMaxLevels) {
        GridLevels lv;
        make_levels(lv, L, S, H);
        binned = make_bin_plan(offsets_host, L, D, lv, align_corners != 0, B).nlev > 0;
    }
    if (!binned) {  // no bin launch to carry the reduce: it goes first, on its own
        if (dw_stash) {
            if (int e = ngp_nerf_dw_reduce(mlp_workspaces, mlp_Bs, in_dims, hidden_dims, num_layers, grad_weights,
                                           mlp_nonfinite, count, dw_stash, dw_stash_rows, dw_rows_max, stream))
                return e;
        } else if (int e = ngp_reduce::launch_slab_reduce(rj, nred, stream)) return e;
        return bwd_fused_impl(grad, xyz, bound, offsets, grad_embeddings, B, count, D, C, L, S, H, gridtype,
                              align_corners, interp, offsets_host, workspace, workspace_bytes, grad_layout,
                              nonfinite, stream, nullptr, 0, &bl, rows);
    }
    return bwd_fused_impl(grad, xyz, bound, offsets, grad_embeddings, B, count, D, C, L, S, H, gridtype,
                          align_corners, interp, offsets_host, workspace, workspace_bytes, grad_layout, nonfinite,
                          stream, &rj, nred, &bl, rows, dw_stash ? &dw : nullptr);
}

extern "C" int ngp_grid_encode_backward_fused_reduce_batch(
    const void* grad, const float* xyz, float bound, const int32_t* offsets, void* grad_embeddings, uint32_t B,
    const int32_t* count, uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H, uint32_t gridtype,
    int32_t align_corners, uint32_t interp, const int32_t* offsets_host, void* workspace, size_t workspace_bytes,
    int32_t grad_layout, int32_t* nonfinite, int32_t n_nets, void* const* mlp_workspaces, const uint32_t* mlp_Bs,
    const uint32_t* in_dims, const uint32_t* hidden_dims, const uint32_t* num_layers, void* const* grad_weights,
    int32_t* mlp_nonfinite, const ngp_batch_job* job, void* stream) {
    return reduce_batch_impl(grad, xyz, bound, offsets, grad_embeddings, B, count, D, C, L, S, H, gridtype,
                             align_corners, interp, offsets_host, workspace, workspace_bytes, grad_layout, nonfinite,
                             n_nets, mlp_workspaces, mlp_Bs, in_dims, hidden_dims, num_layers, grad_weights,
                             mlp_nonfinite, job, stream, nullptr);
}

extern "C" int ngp_grid_encode_backward_fused_reduce_batch_live(
    const void* grad, const float* xyz, float bound, const int32_t* offsets, void* grad_embeddings, uint32_t B,
    const int32_t* live_rows, const int32_t* live_count, uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H,
    uint32_t gridtype, int32_t align_corners, uint32_t interp, const int32_t* offsets_host, void* workspace,
    size_t workspace_bytes, int32_t grad_layout, int32_t* nonfinite, int32_t n_nets, void* const* mlp_workspaces,
    const uint32_t* mlp_Bs, const uint32_t* in_dims, const uint32_t* hidden_dims, const uint32_t* num_layers,
    void* const* grad_weights, int32_t* mlp_nonfinite, const ngp_batch_job* job, void* stream) {
    NGP_REQUIRE(live_rows && live_count, NGP_ERR_ARG, "grid_encode_backward_fused_reduce_batch_live: null row list");
    return reduce_batch_impl(grad, xyz, bound, offsets, grad_embeddings, B, live_count, D, C, L, S, H, gridtype,
                             align_corners, interp, offsets_host, workspace, workspace_bytes, grad_layout, nonfinite,
                             n_nets, mlp_workspaces, mlp_Bs, in_dims, hidden_dims, num_layers, grad_weights,
                             mlp_nonfinite, job, stream, live_rows);
}

extern "C" int ngp_grid_encode_backward_fused_reduce_batch_images(
    const void* grad, const float* xyz, float bound, const int32_t* offsets, void* grad_embeddings, uint32_t B,
    const int32_t* live_rows, const int32_t* live_count, uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H,
    uint32_t gridtype, int32_t align_corners, uint32_t interp, const int32_t* offsets_host, void* workspace,
    size_t workspace_bytes, int32_t grad_layout, int32_t* nonfinite, int32_t n_nets, void* const* mlp_workspaces,
    const uint32_t* mlp_Bs, const uint32_t* in_dims, const uint32_t* hidden_dims, const uint32_t* num_layers,
    void* const* grad_weights, int32_t* mlp_nonfinite, const ngp_batch_job* job, const ngp_image_source* src,
    void* stream) {
    if (int e = ngp_head::check_image_source(src, "grid_encode_backward_fused_reduce_batch_images")) return e;
    if (job)
        if (int e = ngp_head::check_error_map_draw(src, job->N, "grid_encode_backward_fused_reduce_batch_images"))
            return e;
    NGP_REQUIRE(!job || (!job->boxes && job->nboxes == 0), NGP_ERR_ARG,
                "grid_encode_backward_fused_reduce_batch_images: an image job carries no boxes");
    return reduce_batch_impl(grad, xyz, bound, offsets, grad_embeddings, B, live_count, D, C, L, S, H, gridtype,
                             align_corners, interp, offsets_host, workspace, workspace_bytes, grad_layout, nonfinite,
                             n_nets, mlp_workspaces, mlp_Bs, in_dims, hidden_dims, num_layers, grad_weights,
                             mlp_nonfinite, job, stream, live_rows, src);
}

extern "C" int ngp_grid_encode_backward_fused_dw_batch_live(
    const void* grad, const float* xyz, float bound, const int32_t* offsets, void* grad_embeddings, uint32_t B,
    const int32_t* live_rows, const int32_t* live_count, uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H,
    uint32_t gridtype, int32_t align_corners, uint32_t interp, const int32_t* offsets_host, void* workspace,
    size_t workspace_bytes, int32_t grad_layout, int32_t* nonfinite, int32_t n_nets, void* const* mlp_workspaces,
    const uint32_t* mlp_Bs, const uint32_t* in_dims, const uint32_t* hidden_dims, const uint32_t* num_layers,
    void* const* grad_weights, int32_t* mlp_nonfinite, const ngp_batch_job* job, const ngp_image_source* src,
    const void* dw_stash, uint32_t dw_stash_rows, uint32_t dw_rows_max, void* stream) {
    NGP_REQUIRE(live_rows && live_count && dw_stash, NGP_ERR_ARG,
                "grid_encode_backward_fused_dw_batch_live: null row list or stash");
    if (src) {  // the next batch from an image source, as ngp_grid_encode_backward_fused_reduce_batch_images
        if (int e = ngp_head::check_image_source(src, "grid_encode_backward_fused_dw_batch_live")) return e;
        if (job)
            if (int e = ngp_head::check_error_map_draw(src, job->N, "grid_encode_backward_fused_dw_batch_live"))
                return e;
        NGP_REQUIRE(!job || (!job->boxes && job->nboxes == 0), NGP_ERR_ARG,
                    "grid_encode_backward_fused_dw_batch_live: an image job carries no boxes");
    }
    return reduce_batch_impl(grad, xyz, bound, offsets, grad_embeddings, B, live_count, D, C, L, S, H, gridtype,
                             align_corners, interp, offsets_host, workspace, workspace_bytes, grad_layout, nonfinite,
                             n_nets, mlp_workspaces, mlp_Bs, in_dims, hidden_dims, num_layers, grad_weights,
                             mlp_nonfinite, job, stream, live_rows, src, dw_stash, dw_stash_rows, dw_rows_max);
}

#ifdef NGP_STAMPS
extern "C" int ngp_debug_stamps(void* buf) {
    return hipMemcpyToSymbol(HIP_SYMBOL(g_stamps), &buf, sizeof(buf)) == hipSuccess ? NGP_OK : NGP_ERR_HIP;
}
#endif
