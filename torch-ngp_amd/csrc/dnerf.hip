// D-NeRF (dynamic scenes): the time-sliced density grid's update and the
// deformation network's input row, gfx950. DESIGN.md 23.
//
// The reference (dnerf/renderer.py update_extra_state :454-555) walks 64 time
// slices x cascades x blocks in Python, reads nonzero() back per slice and
// cascade in a partial update, packs each slice with a call of its own and
// takes one global mean. Here an update is three device steps with no host
// round trip between them, over the whole grid [T, C, H^3] (a cell's flat
// index is (t * C + c) * H^3 + morton3D(cell)):
//
//   k_dnerf_points    the query points [lo, hi) of an update: world xyz with
//                     the fp32 operations of ngp_density_grid_points, a time
//                     inside the point's slice, the flat cell index. A pure
//                     function of (seed, update, point) through the counter
//                     RNG, in a domain of its own. Partial updates draw, per
//                     slice and cascade, N = H^3 / 4 uniform cells and N cells
//                     out of the occupied list (k_dnerf_occ_*: count per 1024
//                     cells, scan, write in cell order, as density_grid.hip).
//   k_dnerf_ema       grid = max(grid * decay, tmp) where both are >= 0, tmp
//                     back to -1, per-block partial sums of clamp(grid, 0) in
//                     double, in a fixed order
//   k_dnerf_pack      every slice's bitfield at min(mean over ALL slices,
//                     density_thresh)
//
//   k_dnerf_encode    [x, sin/cos(2^f x) f < 10, t, sin/cos(2^f t) f < 6] as
//                     one row of 63 + 13 columns, float or half, with accurate
//                     sinf / cosf (the argument reaches 2^9 bound, where the
//                     hardware sine's error is ~1e-4)
#include "ngp_common.h"

#include <algorithm>

namespace {

constexpr uint32_t kMaxCascades = 16;
constexpr uint32_t kMaxSlices = 1024;

NGP_DEV uint32_t expand_bits(uint32_t v) {
    v = (v * 0x00010001u) & 0xFF0000FFu;
    v = (v * 0x00000101u) & 0x0F00F00Fu;
    v = (v * 0x00000011u) & 0xC30C30C3u;
    v = (v * 0x00000005u) & 0x49249249u;
    return v;
}
NGP_DEV uint32_t morton3(uint32_t x, uint32_t y, uint32_t z) {
    return expand_bits(x) | (expand_bits(y) << 1) | (expand_bits(z) << 2);
}
NGP_DEV uint32_t compact_bits(uint32_t x) {
    x &= 0x09249249u;
    x = (x ^ (x >> 2)) & 0x030C30C3u;
    x = (x ^ (x >> 4)) & 0x0300F00Fu;
    x = (x ^ (x >> 8)) & 0xFF0000FFu;
    x = (x ^ (x >> 16)) & 0x000003FFu;
    return x;
}

// counter-based RNG (density_grid.hip's)
NGP_DEV uint32_t mix32(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352du;
    x ^= x >> 15; x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}
NGP_DEV uint32_t rng_u32(uint32_t seed, uint32_t a, uint32_t b, uint32_t c) {
    return mix32(seed ^ mix32(a + 0x9e3779b9u * mix32(b ^ mix32(c + 0x85ebca6bu))));
}
NGP_DEV float rng_unit(uint32_t seed, uint32_t a, uint32_t b, uint32_t c) {
    return (float)(rng_u32(seed, a, b, c) >> 8) * (1.0f / 16777216.0f);
}

// The draws' own RNG domain (the static grid's is 0xd3a5b1c7): the seed is
// XORed with this tag. Streams: 1..3 position noise, 4 time noise, 7 the
// occupied draw, 8..10 the uniform cell.
constexpr uint32_t kDnerfRngDomain = 0x6b8f2e15u;

struct CascadeScales {
    float s[kMaxCascades];    // float(bound_c - hgs)
    float hgs[kMaxCascades];  // float(bound_c / H)
};

static CascadeScales cascade_scales(uint32_t C, uint32_t H, float bound) {
    CascadeScales cs{};
    for (uint32_t c = 0; c < C && c < kMaxCascades; ++c) {
        const double bc = std::min((double)(1u << c), (double)bound);
        const double hgs = bc / (double)H;
        cs.s[c] = (float)(bc - hgs);
        cs.hgs[c] = (float)hgs;
    }
    return cs;
}

// 1 <= T <= 1024 slices of 1..16 cascades of H^3 cells, H a power of two in
// [2, 1024], every cell countable in 32 bits
static bool grid_shape_ok(uint32_t T, uint32_t C, uint32_t H) {
    return T >= 1 && T <= kMaxSlices && C >= 1 && C <= kMaxCascades && H >= 2 && H <= 1024 && (H & (H - 1)) == 0 &&
           (uint64_t)T * C * H * H * H <= 0xffffffffull;
}

// ---- occupied cells of the segments (slice, cascade) of a partial update ------
constexpr uint32_t kOccBlock = 1024;

// blockIdx.y: segment seg0 + y
__global__ void __launch_bounds__(kOccBlock)
k_dnerf_occ_count(const float* __restrict__ grid, uint32_t H3, uint32_t seg0, uint32_t nblk,
                  uint32_t* __restrict__ bcount) {
    __shared__ uint32_t wc[kOccBlock / 64];
    const uint32_t seg = seg0 + blockIdx.y;
    const uint32_t i = blockIdx.x * kOccBlock + threadIdx.x;
    const bool occ = i < H3 && grid[(size_t)seg * H3 + i] > 0.0f;
    const uint64_t m = __ballot(occ);
    if ((threadIdx.x & 63) == 0) wc[threadIdx.x >> 6] = (uint32_t)__popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t s = 0;
#pragma unroll
        for (uint32_t w = 0; w < kOccBlock / 64; ++w) s += wc[w];
        bcount[(size_t)seg * nblk + blockIdx.x] = s;
    }
}

// One workgroup per segment: exclusive scan of its block counts in place;
// total[seg] = its occupied cells.
__global__ void __launch_bounds__(1024)
k_dnerf_occ_scan(uint32_t* __restrict__ bcount, uint32_t nblk, uint32_t seg0, uint32_t* __restrict__ total) {
    __shared__ uint32_t wsum[16];
    __shared__ uint32_t carry;
    const uint32_t seg = seg0 + blockIdx.x, t = threadIdx.x, lane = t & 63, wv = t >> 6;
    uint32_t* bc = bcount + (size_t)seg * nblk;
    if (t == 0) carry = 0;
    __syncthreads();
    for (uint32_t base = 0; base < nblk; base += 1024) {
        const uint32_t v = base + t < nblk ? bc[base + t] : 0u;
        uint32_t incl = v;
#pragma unroll
        for (uint32_t o = 1; o < 64; o <<= 1) {
            const uint32_t u = __shfl_up(incl, o, 64);
            if (lane >= o) incl += u;
        }
        if (lane == 63) wsum[wv] = incl;
        __syncthreads();
        uint32_t before = carry, all = 0;
#pragma unroll
        for (uint32_t w = 0; w < 16; ++w) {
            before += w < wv ? wsum[w] : 0u;
            all += wsum[w];
        }
        if (base + t < nblk) bc[base + t] = before + incl - v;
        __syncthreads();
        if (t == 0) carry += all;
        __syncthreads();
    }
    if (t == 0) total[seg] = carry;
}

__global__ void __launch_bounds__(kOccBlock)
k_dnerf_occ_write(const float* __restrict__ grid, uint32_t H3, uint32_t seg0, uint32_t nblk,
                  const uint32_t* __restrict__ bcount, uint32_t* __restrict__ occ) {
    __shared__ uint32_t wc[kOccBlock / 64];
    const uint32_t seg = seg0 + blockIdx.y;
    const uint32_t i = blockIdx.x * kOccBlock + threadIdx.x;
    const bool o = i < H3 && grid[(size_t)seg * H3 + i] > 0.0f;
    const uint64_t m = __ballot(o);
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) wc[wv] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t before = bcount[(size_t)seg * nblk + blockIdx.x];
    for (uint32_t w = 0; w < wv; ++w) before += wc[w];
    const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    // before + below < the segment's occupied cells <= H3: inside the segment's H3 slots
    if (o) occ[(size_t)seg * H3 + before + below] = i;
}

struct PointPlan {
    uint32_t T, C, H, H3;
    uint32_t pps;           // points per segment: H^3 (full) or 2 * (H^3 / 4)
    uint32_t seed, update;  // seed: already XORed with kDnerfRngDomain
    const uint32_t* occ;    // partial: occupied cells of each segment, cell order
    const uint32_t* total;  // partial: their counts
};

// Point p = lo + i of the update: segment p / pps (slice-major, then cascade).
__global__ void __launch_bounds__(256)
k_dnerf_points(PointPlan pl, bool partial, uint32_t lo, uint32_t n, CascadeScales cs, float* __restrict__ xyzs,
               float* __restrict__ times, int32_t* __restrict__ indices) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t p = lo + i;  // < T * C * pps <= 2^32 - 1
    const uint32_t seg = p / pl.pps, k = p - seg * pl.pps;
    const uint32_t t = seg / pl.C, cas = seg - t * pl.C;
    uint32_t cell;
    if (!partial) {
        cell = k;  // point p is cell p
    } else {
        const uint32_t half = pl.pps / 2;
        const uint32_t n_occ = pl.total[seg];
        if (k >= half && n_occ > 0) {
            cell = pl.occ[(size_t)seg * pl.H3 + rng_u32(pl.seed, pl.update, p, 7) % n_occ];
        } else {
            // H a power of two: % H keeps the low bits, the cell stays below H^3
            cell = morton3(rng_u32(pl.seed, pl.update, p, 8) % pl.H, rng_u32(pl.seed, pl.update, p, 9) % pl.H,
                           rng_u32(pl.seed, pl.update, p, 10) % pl.H);
        }
    }
    const uint32_t c[3] = {compact_bits(cell), compact_bits(cell >> 1), compact_bits(cell >> 2)};
    const float inv = 1.0f / (float)(pl.H - 1);
    const float s = cs.s[cas], h = cs.hgs[cas];
#pragma unroll
    for (int j = 0; j < 3; ++j) {  // k_density_points' arithmetic
        float x = 2.0f * (float)c[j];
        x = x * inv;
        x = x - 1.0f;
        x = x * s;
        float jt = rng_unit(pl.seed, pl.update, p, 1 + j) * 2.0f;
        jt = jt - 1.0f;
        jt = jt * h;
        xyzs[(size_t)i * 3 + j] = x + jt;
    }
    // time = (t + 0.5) / T + (2 u - 1) * 0.5 / T, kept inside the slice
    // [t / T, (t + 1) / T] as float32 evaluates its ends (the sum's rounding
    // can step one ulp past them)
    const float fT = (float)pl.T;
    const float centre = ((float)t + 0.5f) / fT, hts = 0.5f / fT;
    float jt = rng_unit(pl.seed, pl.update, p, 4) * 2.0f;
    jt = jt - 1.0f;
    jt = jt * hts;
    float tm = centre + jt;
    tm = fminf(fmaxf(tm, (float)t / fT), (float)(t + 1) / fT);
    times[i] = tm;
    indices[i] = (int32_t)(seg * pl.H3 + cell);
}

NGP_DEV float torch_maximum(float a, float b) {  // torch.maximum: NaN propagates
    if (__builtin_isnan(a) || __builtin_isnan(b)) return __builtin_nanf("");
    return a > b ? a : b;
}

constexpr uint32_t kEmaThreads = 256;
constexpr uint32_t kEmaMaxBlocks = 1024;  // NGP_DNERF_STATS_LEN - 1

// Cells i0, i0 + stride, ... per thread (64-bit: n reaches 2^32 - 1), U loads
// in flight, the adds in cell order; a block's partial sum in a fixed order.
__global__ void __launch_bounds__(kEmaThreads)
k_dnerf_ema(float* __restrict__ grid, float* __restrict__ tmp, uint64_t n, float decay,
            double* __restrict__ partial) {
    __shared__ double wsum[kEmaThreads / 64];
    double acc = 0.0;
    constexpr uint32_t U = 4;
    const uint64_t stride = (uint64_t)gridDim.x * kEmaThreads;
    for (uint64_t i0 = (uint64_t)blockIdx.x * kEmaThreads + threadIdx.x; i0 < n; i0 += U * stride) {
        float gv[U], tv[U];
#pragma unroll
        for (uint32_t u = 0; u < U; ++u) {
            const uint64_t i = min(i0 + u * stride, n - 1);
            gv[u] = grid[i];
            tv[u] = tmp[i];
        }
#pragma unroll
        for (uint32_t u = 0; u < U; ++u) {
            const uint64_t i = i0 + u * stride;
            if (i >= n) break;
            float g = gv[u];
            const float t = tv[u];
            if (g >= 0 && t >= 0) {
                g = torch_maximum(g * decay, t);
                grid[i] = g;
            }
            tmp[i] = -1.0f;
            acc += g < 0 ? 0.0 : (double)g;  // clamp(min=0); NaN stays NaN
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double b = 0.0;
#pragma unroll
        for (uint32_t w = 0; w < kEmaThreads / 64; ++w) b += wsum[w];
        partial[blockIdx.x] = b;
    }
}

// Every slice's bits at thresh = min(mean_density, density_thresh), the mean
// over the whole [T, C, H^3] grid (Python's min: a NaN mean stays NaN and
// clears every bit). Every block adds the partial sums up in the same order.
__global__ void __launch_bounds__(256)
k_dnerf_pack(const float* __restrict__ grid, uint32_t nbytes, uint64_t n, const double* __restrict__ partial,
             uint32_t nparts, double density_thresh, uint8_t* __restrict__ bitfield, double* __restrict__ stats) {
    __shared__ double s_sum[256];
    double acc = 0.0;
    for (uint32_t i = threadIdx.x; i < nparts; i += 256) acc += partial[i];
    s_sum[threadIdx.x] = acc;
    __syncthreads();
    for (uint32_t o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) s_sum[threadIdx.x] += s_sum[threadIdx.x + o];
        __syncthreads();
    }
    const double sum = s_sum[0];
    if (blockIdx.x == 0 && threadIdx.x == 0) stats[0] = sum;
    const uint32_t b = blockIdx.x * 256 + threadIdx.x;
    if (b >= nbytes) return;
    const double mean = (double)(float)(sum / (double)n);
    const float thresh = (float)(density_thresh < mean ? density_thresh : mean);
    const float4* g = reinterpret_cast<const float4*>(grid + (size_t)b * 8);
    const float4 a = g[0], c = g[1];
    uint32_t bits = 0;
    bits |= (a.x > thresh) ? 1u : 0u;
    bits |= (a.y > thresh) ? 2u : 0u;
    bits |= (a.z > thresh) ? 4u : 0u;
    bits |= (a.w > thresh) ? 8u : 0u;
    bits |= (c.x > thresh) ? 16u : 0u;
    bits |= (c.y > thresh) ? 32u : 0u;
    bits |= (c.z > thresh) ? 64u : 0u;
    bits |= (c.w > thresh) ? 128u : 0u;
    bitfield[b] = (uint8_t)bits;
}

// ---- the deformation network's input row ------------------------------------------
constexpr uint32_t kEncXDeg = 10, kEncTDeg = 6;
constexpr uint32_t kEncXCols = 3 + 6 * kEncXDeg;  // 63
constexpr uint32_t kEncTCols = 1 + 2 * kEncTDeg;  // 13
constexpr uint32_t kEncCols = kEncXCols + kEncTCols;

// One output element per thread, consecutive lanes on consecutive columns of
// a row (freqencoder.hip's column order: the input, then per octave the sines
// of every coordinate, then the cosines).
template <typename O>
__global__ void __launch_bounds__(256)
k_dnerf_encode(const float* __restrict__ x, const float* __restrict__ t, uint32_t t_stride, uint32_t total,
               O* __restrict__ out, uint32_t row_stride) {
    const uint32_t e = blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const uint32_t b = e / kEncCols, c = e - b * kEncCols;
    float v;
    if (c < kEncXCols) {
        const float* row = x + (size_t)b * 3;
        if (c < 3) {
            v = row[c];
        } else {
            const uint32_t col = c / 3 - 1, d = c - (col + 1) * 3;
            const float a = scalbnf(row[d], (int)(col >> 1));  // exact
            v = (col & 1u) ? cosf(a) : sinf(a);
        }
    } else {
        const float tv = t[(size_t)b * t_stride];
        const uint32_t ct = c - kEncXCols;
        if (ct == 0) {
            v = tv;
        } else {
            const uint32_t col = ct - 1;
            const float a = scalbnf(tv, (int)(col >> 1));
            v = (col & 1u) ? cosf(a) : sinf(a);
        }
    }
    if constexpr (sizeof(O) == 2) {
        out[(size_t)b * row_stride + c] = ngp_f2h(v);
    } else {
        out[(size_t)b * row_stride + c] = v;
    }
}

}  // namespace

extern "C" int ngp_dnerf_encode(const float* x, const float* t, uint32_t t_stride, uint32_t N, void* out,
                                int32_t out_dtype, uint32_t row_stride, void* stream) {
    NGP_REQUIRE(t_stride <= 1, NGP_ERR_ARG, "dnerf_encode: the time's element stride must be 0 or 1, got %u", t_stride);
    NGP_REQUIRE(out_dtype == NGP_DTYPE_F32 || out_dtype == NGP_DTYPE_F16, NGP_ERR_ARG,
                "dnerf_encode: the output must be float32 or float16, got dtype code %d", out_dtype);
    NGP_REQUIRE(row_stride >= kEncCols, NGP_ERR_ARG, "dnerf_encode: row stride %u below the row's %u columns", row_stride,
                kEncCols);
    NGP_REQUIRE((uint64_t)N * kEncCols < (1ull << 32) - 256, NGP_ERR_ARG,
                "dnerf_encode: N * %u must stay below 2^32, got N = %u", kEncCols, N);
    if (N == 0) return NGP_OK;
    NGP_REQUIRE(x && t && out, NGP_ERR_ARG, "dnerf_encode: null x / t / out");
    const uint32_t total = N * kEncCols;
    hipStream_t st = ngp_stream(stream);
    if (out_dtype == NGP_DTYPE_F16) {
        k_dnerf_encode<ngp_half><<<ngp_div_up(total, 256), 256, 0, st>>>(x, t, t_stride, total,
                                                                         static_cast<ngp_half*>(out), row_stride);
    } else {
        k_dnerf_encode<float><<<ngp_div_up(total, 256), 256, 0, st>>>(x, t, t_stride, total, static_cast<float*>(out),
                                                                      row_stride);
    }
    return ngp_check_launch("dnerf_encode");
}

// bcount [segs * nblk], total [segs], padded to 256 bytes, then occ [segs * H^3]
static size_t occ_header_bytes(uint32_t segs, uint32_t nblk) {
    return (((size_t)segs * nblk + segs) * sizeof(uint32_t) + 255) / 256 * 256;
}

extern "C" size_t ngp_dnerf_grid_points_workspace_bytes(uint32_t T, uint32_t C, uint32_t H) {
    if (!grid_shape_ok(T, C, H)) return 0;
    const uint32_t H3 = H * H * H, segs = T * C;
    return occ_header_bytes(segs, ngp_div_up(H3, kOccBlock)) + (size_t)segs * H3 * sizeof(uint32_t);
}

extern "C" int ngp_dnerf_grid_points(const float* grid, uint32_t T, uint32_t C, uint32_t H, float bound,
                                     uint32_t partial, uint32_t seed, uint32_t update, uint32_t lo, uint32_t hi,
                                     void* ws, size_t ws_bytes, float* xyzs, float* times, int32_t* indices,
                                     void* stream) {
    NGP_REQUIRE(grid_shape_ok(T, C, H), NGP_ERR_ARG,
                "dnerf_grid_points: %u slices / %u cascades / grid size %u (a power of two) out of range", T, C, H);
    NGP_REQUIRE(bound > 0.0f, NGP_ERR_ARG, "dnerf_grid_points: bound must be positive");
    const uint32_t H3 = H * H * H, segs = T * C;
    const uint32_t pps = partial ? 2 * (H3 / 4) : H3;
    const uint64_t P = (uint64_t)segs * pps;
    NGP_REQUIRE(lo <= hi && hi <= P, NGP_ERR_ARG, "dnerf_grid_points: [%u, %u) outside the update's %llu points", lo, hi,
                (unsigned long long)P);
    if (hi == lo) return NGP_OK;
    NGP_REQUIRE(xyzs && times && indices, NGP_ERR_ARG, "dnerf_grid_points: null xyzs / times / indices");
    NGP_REQUIRE(!partial || (grid && ws), NGP_ERR_ARG, "dnerf_grid_points: a partial update needs the grid and a workspace");
    NGP_REQUIRE(!partial || ws_bytes >= ngp_dnerf_grid_points_workspace_bytes(T, C, H), NGP_ERR_ARG,
                "dnerf_grid_points: workspace of %zu bytes required, got %zu",
                ngp_dnerf_grid_points_workspace_bytes(T, C, H), ws_bytes);
    hipStream_t st = ngp_stream(stream);
    PointPlan pl{T, C, H, H3, pps, seed ^ kDnerfRngDomain, update, nullptr, nullptr};
    if (partial) {
        // the occupied lists of the segments [lo, hi) touches (each update's
        // ranges cover a segment once when they end on segment boundaries)
        const uint32_t nblk = ngp_div_up(H3, kOccBlock);
        const uint32_t seg0 = lo / pps, seg1 = (hi - 1) / pps, nseg = seg1 - seg0 + 1;  // nseg <= 16384
        uint32_t* bcount = static_cast<uint32_t*>(ws);
        uint32_t* total = bcount + (size_t)segs * nblk;
        uint32_t* occ = reinterpret_cast<uint32_t*>(static_cast<char*>(ws) + occ_header_bytes(segs, nblk));
        k_dnerf_occ_count<<<dim3(nblk, nseg), kOccBlock, 0, st>>>(grid, H3, seg0, nblk, bcount);
        k_dnerf_occ_scan<<<nseg, 1024, 0, st>>>(bcount, nblk, seg0, total);
        k_dnerf_occ_write<<<dim3(nblk, nseg), kOccBlock, 0, st>>>(grid, H3, seg0, nblk, bcount, occ);
        pl.occ = occ;
        pl.total = total;
    }
    k_dnerf_points<<<ngp_div_up(hi - lo, 256), 256, 0, st>>>(pl, partial != 0, lo, hi - lo,
                                                            cascade_scales(C, H, bound), xyzs, times, indices);
    return ngp_check_launch("dnerf_grid_points");
}

extern "C" int ngp_dnerf_grid_ema_pack(float* grid, float* tmp_grid, uint32_t T, uint32_t C, uint32_t H, float decay,
                                       double density_thresh, double* stats, uint8_t* bitfield, void* stream) {
    NGP_REQUIRE(grid_shape_ok(T, C, H), NGP_ERR_ARG,
                "dnerf_grid_ema_pack: %u slices / %u cascades / grid size %u (a power of two) out of range", T, C, H);
    NGP_REQUIRE(grid && tmp_grid && stats && bitfield, NGP_ERR_ARG, "dnerf_grid_ema_pack: null pointer");
    NGP_REQUIRE(((uintptr_t)grid & 15u) == 0, NGP_ERR_ARG, "dnerf_grid_ema_pack: the grid must be 16-byte aligned");
    const uint64_t n = (uint64_t)T * C * H * H * H;  // a multiple of 8
    hipStream_t st = ngp_stream(stream);
    // stats: [0] the sum, [1..] the EMA blocks' partial sums
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((n + kEmaThreads - 1) / kEmaThreads, kEmaMaxBlocks);
    k_dnerf_ema<<<blocks, kEmaThreads, 0, st>>>(grid, tmp_grid, n, decay, stats + 1);
    const uint32_t nbytes = (uint32_t)(n / 8);
    k_dnerf_pack<<<ngp_div_up(nbytes, 256), 256, 0, st>>>(grid, nbytes, n, stats + 1, blocks, density_thresh, bitfield,
                                                         stats);
    return ngp_check_launch("dnerf_grid_ema_pack");
}
