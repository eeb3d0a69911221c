// TensoRF's vector-matrix (VM) decomposition: the encoder of main_tensoRF.py.
//
// A field component i is a plane over two axes times a line over the third,
//   feat_i[r](x) = plane_i[r](u, v) * line_i[r](w),   r < R_i,
// with (u, v) = x[mat_ids[i]], mat_ids = (0,1) (0,2) (1,2) (W along the first,
// H along the second) and w = x[vec_ids[i]], vec_ids = 2 1 0. The reference
// (tensoRF/network.py:112-153) samples every plane and line with its own
// F.grid_sample(bilinear, zeros, align_corners=True) call on [1, R, H, W] and
// [1, R, D, 1] textures. Here a plane is stored [H, W, R] and a line [D, R],
// so one bilinear corner is R contiguous floats, and
//
//   ngp_vm_forward   normalises x into aabb_train and gives, per set of three
//                    planes and lines, the sum over i and r (`sum`, the
//                    density feature) or the products themselves (`concat`,
//                    the colour features), for one or two sets per call;
//   ngp_vm_backward  recomputes the interpolation from x and scatters the
//                    gradients of every plane and line. Each contribution is
//                    rounded to a fixed-point quantum and added with 64-bit
//                    integer atomics (a line's through an LDS copy per
//                    workgroup first), so the sums do not depend on the
//                    arrival order: two runs give the same bits. The quantum
//                    is 2^-32 of the smallest power of two above the call's
//                    largest |output gradient| (found by a first launch), so
//                    it follows the GradScaler's scale exactly.
//
// Sixteen lanes share a point and run over r, so every load, store and atomic
// of a group is one contiguous run of up to 64 bytes. Plain C++ HIP, vector
// stores only. DESIGN.md 22.
#include "ngp_common.h"

#include <cmath>

namespace {

typedef unsigned long long fixed_t;

constexpr uint32_t kThreads = 256;
constexpr uint32_t kGroup = 16;                    // lanes per point (over r)
constexpr uint32_t kPoints = kThreads / kGroup;    // points per workgroup pass
constexpr uint32_t kChunkPoints = 2048;            // points per backward workgroup
constexpr uint32_t kLdsLine = 512;                 // longest line summed in LDS: 512 * 16 * 8 B = 64 KiB
constexpr uint32_t kHdrWords = 4;                  // scratch header: max |g| bits, bad flag, 2 unused (16 B)
constexpr double kFixedLimit = 1099511627776.0;    // 2^40 quanta per contribution: 2^22 points fit 2^62
constexpr int kFixedBits = NGP_VM_FIXED_BITS;

struct VmParams {
    const float* plane[2][3];
    const float* line[2][3];
    uint32_t rank[2][3];
    uint32_t roff[2][3];  // column of component i in the concat row
    uint32_t width[2];    // sum of the ranks
    uint32_t res[3];
    unsigned long long poff[2][3], loff[2][3];  // where each gradient starts, in values
};

// One axis of grid_sample(bilinear, zeros, align_corners=True) on `size`
// texels: the two texels and their weights in torch's operation order. An
// index outside the texture has v = false (its texel counts as zero); i is
// clamped into the texture so that every address formed from it is valid.
struct Lin {
    uint32_t i0, i1;
    float w0, w1;
    bool v0, v1;
};

NGP_DEV Lin lin_setup(float c, uint32_t size) {
    float f = ((c + 1.0f) / 2.0f) * (float)(size - 1);
    // past these every texel is outside anyway; a NaN becomes -2 (zero output)
    f = fminf(fmaxf(f, -2.0f), (float)size + 1.0f);
    const float fl = floorf(f);
    const int i = (int)fl, last = (int)size - 1;
    Lin l;
    l.w1 = f - fl;
    l.w0 = (fl + 1.0f) - f;
    l.v0 = i >= 0 && i <= last;
    l.v1 = i + 1 >= 0 && i + 1 <= last;
    l.i0 = (uint32_t)min(max(i, 0), last);
    l.i1 = (uint32_t)min(max(i + 1, 0), last);
    return l;
}

NGP_DEV int mat_axis0(int i) { return i == 2 ? 1 : 0; }
NGP_DEV int mat_axis1(int i) { return i == 0 ? 1 : 2; }
NGP_DEV int vec_axis(int i) { return 2 - i; }

// 2 * (x - lo) / (hi - lo) - 1 in float32, in that order
NGP_DEV void normalise(const float* __restrict__ x, size_t n, const float* __restrict__ aabb, float c[3]) {
    for (int a = 0; a < 3; ++a) {
        const float lo = aabb[a], hi = aabb[a + 3];
        const float t = 2.0f * (x[n * 3 + a] - lo);
        c[a] = t / (hi - lo) - 1.0f;
    }
}

struct Taps {
    Lin x, y, z;
    uint32_t W;
};

NGP_DEV Taps taps_of(const VmParams& P, int i, const float c[3]) {
    Taps t;
    const int a0 = mat_axis0(i), a1 = mat_axis1(i), av = vec_axis(i);
    t.x = lin_setup(c[a0], P.res[a0]);
    t.y = lin_setup(c[a1], P.res[a1]);
    t.z = lin_setup(c[av], P.res[av]);
    t.W = P.res[a0];
    return t;
}

NGP_DEV float plane_at(const float* __restrict__ pl, const Taps& t, uint32_t R, uint32_t r) {
    const float v00 = pl[((size_t)t.y.i0 * t.W + t.x.i0) * R + r], v01 = pl[((size_t)t.y.i0 * t.W + t.x.i1) * R + r];
    const float v10 = pl[((size_t)t.y.i1 * t.W + t.x.i0) * R + r], v11 = pl[((size_t)t.y.i1 * t.W + t.x.i1) * R + r];
    float p = (t.x.v0 && t.y.v0 ? v00 : 0.0f) * (t.x.w0 * t.y.w0);
    p += (t.x.v1 && t.y.v0 ? v01 : 0.0f) * (t.x.w1 * t.y.w0);
    p += (t.x.v0 && t.y.v1 ? v10 : 0.0f) * (t.x.w0 * t.y.w1);
    p += (t.x.v1 && t.y.v1 ? v11 : 0.0f) * (t.x.w1 * t.y.w1);
    return p;
}

NGP_DEV float line_at(const float* __restrict__ ln, const Taps& t, uint32_t R, uint32_t r) {
    const float t0 = ln[(size_t)t.z.i0 * R + r], t1 = ln[(size_t)t.z.i1 * R + r];
    float l = (t.z.v0 ? t0 : 0.0f) * t.z.w0;
    l += (t.z.v1 ? t1 : 0.0f) * t.z.w1;
    return l;
}

// Set s of P at 16 points per workgroup. SUM: out f32 [N]; else f32 [N, width].
template <bool SUM>
__global__ void __launch_bounds__(kThreads)
k_vm_forward(VmParams P, int s, const float* __restrict__ x, uint32_t N, const float* __restrict__ aabb,
             float* __restrict__ out) {
    const uint32_t lane = threadIdx.x % kGroup;
    const size_t slot = (size_t)blockIdx.x * kPoints + threadIdx.x / kGroup;
    const bool live = slot < N;
    const size_t n = live ? slot : (size_t)N - 1;  // (every lane takes part in the shuffles)
    float c[3];
    normalise(x, n, aabb, c);
    float acc = 0.0f;
    for (int i = 0; i < 3; ++i) {
        const Taps t = taps_of(P, i, c);
        const uint32_t R = P.rank[s][i];
        for (uint32_t r = lane; r < R; r += kGroup) {
            const float v = plane_at(P.plane[s][i], t, R, r) * line_at(P.line[s][i], t, R, r);
            if (SUM)
                acc += v;
            else if (live)
                out[n * P.width[s] + P.roff[s][i] + r] = v;
        }
    }
    if (SUM) {
        for (int m = kGroup / 2; m >= 1; m >>= 1) acc += __shfl_xor(acc, m, kGroup);
        if (live && lane == 0) out[n] = acc;
    }
}

// hdr[0] = max over both gradients of the bits of |g| (a NaN or an infinity
// compares above every finite value)
__global__ void __launch_bounds__(kThreads)
k_vm_gmax(const float* __restrict__ a, size_t na, const float* __restrict__ b, size_t nb, uint32_t* __restrict__ hdr) {
    uint32_t m = 0;
    const size_t stride = (size_t)gridDim.x * kThreads;
    for (size_t k = (size_t)blockIdx.x * kThreads + threadIdx.x; k < na; k += stride)
        m = max(m, __float_as_uint(a[k]) & 0x7fffffffu);
    for (size_t k = (size_t)blockIdx.x * kThreads + threadIdx.x; k < nb; k += stride)
        m = max(m, __float_as_uint(b[k]) & 0x7fffffffu);
    for (int w = 32; w >= 1; w >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, w, 64));
    if (threadIdx.x % 64 == 0 && m != 0) atomicMax(hdr, m);
}

// The smallest power of two above a finite float with bits gb, as an exponent.
NGP_DEV int exponent_above(uint32_t gb) { return max((int)(gb >> 23), 1) - 126; }

// *p += v in quanta; false when v does not fit (nothing is added then)
NGP_DEV bool add_fixed(fixed_t* p, float v, double qinv) {  // (p in global memory or in LDS)
    const double d = (double)v * qinv;
    if (!(fabs(d) < kFixedLimit)) return false;
    const long long q = __double2ll_rn(d);
    if (q != 0) atomicAdd(p, (fixed_t)q);
    return true;
}

// Workgroup (bx, by): points [bx * kChunkPoints, ...), and the by-th chunk of
// 16 ranks of one component of one set. Its plane gradients go straight to
// the scratch; its line gradients are summed in LDS (D x 16 accumulators) and
// added to the scratch once at the end. A line longer than kLdsLine texels
// is added straight to the scratch as well.
__global__ void __launch_bounds__(kThreads)
k_vm_backward(VmParams P, const float* __restrict__ x, uint32_t N, const float* __restrict__ aabb,
              const float* __restrict__ gsum, const float* __restrict__ gcat, uint32_t* __restrict__ hdr,
              fixed_t* __restrict__ scratch) {
    extern __shared__ fixed_t lds[];
    const uint32_t gb = hdr[0];
    if (gb == 0 || gb >= 0x7f800000u) return;  // nothing to add; or not finite: k_vm_finish writes NaN
    const double qinv = ldexp(1.0, kFixedBits - exponent_above(gb));

    // the job of this row of workgroups
    int s = 0, i = 0;
    uint32_t j = blockIdx.y;
    bool found = false;
    for (int ss = 0; ss < 2 && !found; ++ss) {
        if (!(ss == 0 ? gsum : gcat)) continue;
        for (int ii = 0; ii < 3 && !found; ++ii) {
            const uint32_t nch = ngp_div_up(P.rank[ss][ii], kGroup);
            if (j < nch) {
                s = ss, i = ii, found = true;
            } else {
                j -= nch;
            }
        }
    }
    if (!found) return;
    const uint32_t R = P.rank[s][i], r0 = j * kGroup;
    const uint32_t rn = min(kGroup, R - r0);
    const uint32_t D = P.res[vec_axis(i)];
    const bool in_lds = D <= kLdsLine;
    if (in_lds) {
        for (uint32_t k = threadIdx.x; k < D * kGroup; k += kThreads) lds[k] = 0;
        __syncthreads();
    }
    fixed_t* gplane = scratch + P.poff[s][i];
    fixed_t* gline = scratch + P.loff[s][i];
    const float* pl = P.plane[s][i];
    const float* ln = P.line[s][i];

    const uint32_t lane = threadIdx.x % kGroup, r = r0 + lane;
    const size_t first = (size_t)blockIdx.x * kChunkPoints;
    const size_t last = first + kChunkPoints < (size_t)N ? first + kChunkPoints : (size_t)N;
    bool bad = false;
    if (lane < rn) {
        for (size_t n = first + threadIdx.x / kGroup; n < last; n += kPoints) {
            const float g = s == 0 ? gsum[n] : gcat[n * P.width[1] + P.roff[1][i] + r];
            if (g == 0.0f) continue;
            float c[3];
            normalise(x, n, aabb, c);
            const Taps t = taps_of(P, i, c);
            const float lg = line_at(ln, t, R, r) * g, pg = plane_at(pl, t, R, r) * g;
            if (t.x.v0 && t.y.v0)
                bad |= !add_fixed(gplane + ((size_t)t.y.i0 * t.W + t.x.i0) * R + r, (t.x.w0 * t.y.w0) * lg, qinv);
            if (t.x.v1 && t.y.v0)
                bad |= !add_fixed(gplane + ((size_t)t.y.i0 * t.W + t.x.i1) * R + r, (t.x.w1 * t.y.w0) * lg, qinv);
            if (t.x.v0 && t.y.v1)
                bad |= !add_fixed(gplane + ((size_t)t.y.i1 * t.W + t.x.i0) * R + r, (t.x.w0 * t.y.w1) * lg, qinv);
            if (t.x.v1 && t.y.v1)
                bad |= !add_fixed(gplane + ((size_t)t.y.i1 * t.W + t.x.i1) * R + r, (t.x.w1 * t.y.w1) * lg, qinv);
            if (t.z.v0)
                bad |= !add_fixed(in_lds ? lds + t.z.i0 * kGroup + lane : gline + (size_t)t.z.i0 * R + r,
                                  t.z.w0 * pg, qinv);
            if (t.z.v1)
                bad |= !add_fixed(in_lds ? lds + t.z.i1 * kGroup + lane : gline + (size_t)t.z.i1 * R + r,
                                  t.z.w1 * pg, qinv);
        }
    }
    if (bad) atomicOr(hdr + 1, 1u);
    if (in_lds) {
        __syncthreads();
        for (uint32_t k = threadIdx.x; k < D * kGroup; k += kThreads) {
            const fixed_t v = lds[k];
            const uint32_t d = k / kGroup, rr = k % kGroup;
            if (v != 0 && rr < rn) atomicAdd(gline + (size_t)d * R + r0 + rr, v);
        }
    }
}

// scratch (quanta) -> float32 gradients; NaN everywhere when a gradient was not finite or did not fit
__global__ void __launch_bounds__(kThreads)
k_vm_finish(const fixed_t* __restrict__ scratch, const uint32_t* __restrict__ hdr, size_t total,
            float* __restrict__ grads) {
    const uint32_t gb = hdr[0];
    const bool bad = gb >= 0x7f800000u || hdr[1] != 0;
    const double quantum = gb == 0 ? 0.0 : ldexp(1.0, exponent_above(gb & 0x7fffffffu) - kFixedBits);
    const size_t stride = (size_t)gridDim.x * kThreads;
    for (size_t k = (size_t)blockIdx.x * kThreads + threadIdx.x; k < total; k += stride)
        grads[k] = bad ? __uint_as_float(0x7fc00000u) : (float)((double)(long long)scratch[k] * quantum);
}

// Checks both sets and lays their gradients out: per set given, planes 0 1 2 then lines 0 1 2.
int make_params(const char* what, uint32_t res0, uint32_t res1, uint32_t res2, const ngp_vm_set* const sets[2],
                VmParams& P, size_t& total) {
    P = VmParams{};
    P.res[0] = res0, P.res[1] = res1, P.res[2] = res2;
    for (int a = 0; a < 3; ++a)
        NGP_REQUIRE(P.res[a] >= 1 && P.res[a] <= NGP_VM_MAX_RES, NGP_ERR_ARG, "%s: resolution %u must be in [1, %u]",
                    what, P.res[a], (unsigned)NGP_VM_MAX_RES);
    total = 0;
    for (int s = 0; s < 2; ++s) {
        if (!sets[s]) continue;
        for (int i = 0; i < 3; ++i) {
            const uint32_t R = sets[s]->rank[i];
            NGP_REQUIRE(R >= 1 && R <= NGP_VM_MAX_RANK, NGP_ERR_ARG, "%s: rank %u must be in [1, %u]", what, R,
                        (unsigned)NGP_VM_MAX_RANK);
            NGP_REQUIRE(sets[s]->plane[i] && sets[s]->line[i], NGP_ERR_ARG, "%s: null plane or line", what);
            P.plane[s][i] = sets[s]->plane[i], P.line[s][i] = sets[s]->line[i];
            P.rank[s][i] = R;
            P.roff[s][i] = P.width[s];
            P.width[s] += R;
        }
        for (int i = 0; i < 3; ++i) {
            P.poff[s][i] = total;
            total += (size_t)P.res[i == 2 ? 1 : 0] * P.res[i == 0 ? 1 : 2] * P.rank[s][i];
        }
        for (int i = 0; i < 3; ++i) {
            P.loff[s][i] = total;
            total += (size_t)P.res[2 - i] * P.rank[s][i];
        }
    }
    return NGP_OK;
}

}  // namespace

extern "C" int ngp_vm_forward(const float* x, uint32_t N, const float* aabb6, uint32_t res0, uint32_t res1,
                              uint32_t res2, const ngp_vm_set* sum_set, float* sigma_feat, const ngp_vm_set* cat_set,
                              float* prod, void* stream) {
    const ngp_vm_set* sets[2] = {sum_set, cat_set};
    VmParams P;
    size_t total;
    const int rc = make_params("vm_forward", res0, res1, res2, sets, P, total);
    if (rc != NGP_OK) return rc;
    NGP_REQUIRE(sum_set || cat_set, NGP_ERR_ARG, "vm_forward: no set");
    NGP_REQUIRE(N < (1u << 30), NGP_ERR_ARG, "vm_forward: N (%u) must be below 2^30", N);
    if (N == 0) return NGP_OK;
    NGP_REQUIRE((!sum_set || sigma_feat) && (!cat_set || prod), NGP_ERR_ARG, "vm_forward: a set without its output");
    NGP_REQUIRE(x && aabb6, NGP_ERR_ARG, "vm_forward: null buffer");
    const uint32_t blocks = ngp_div_up(N, kPoints);
    if (sum_set) {
        k_vm_forward<true><<<blocks, kThreads, 0, ngp_stream(stream)>>>(P, 0, x, N, aabb6, sigma_feat);
        const int rl = ngp_check_launch("vm_forward (sum)");
        if (rl != NGP_OK) return rl;
    }
    if (cat_set) {
        k_vm_forward<false><<<blocks, kThreads, 0, ngp_stream(stream)>>>(P, 1, x, N, aabb6, prod);
        return ngp_check_launch("vm_forward (concat)");
    }
    return NGP_OK;
}

extern "C" size_t ngp_vm_grad_values(uint32_t res0, uint32_t res1, uint32_t res2, const ngp_vm_set* sum_set,
                                     const ngp_vm_set* cat_set) {
    const ngp_vm_set* sets[2] = {sum_set, cat_set};
    VmParams P;
    size_t total = 0;
    if (make_params("vm_grad_values", res0, res1, res2, sets, P, total) != NGP_OK) return 0;
    return total;
}

extern "C" size_t ngp_vm_backward_scratch_bytes(uint32_t res0, uint32_t res1, uint32_t res2,
                                                const ngp_vm_set* sum_set, const ngp_vm_set* cat_set) {
    const size_t total = ngp_vm_grad_values(res0, res1, res2, sum_set, cat_set);
    return total ? kHdrWords * sizeof(uint32_t) + total * sizeof(fixed_t) : 0;
}

extern "C" int ngp_vm_backward(const float* x, uint32_t N, const float* aabb6, uint32_t res0, uint32_t res1,
                               uint32_t res2, const ngp_vm_set* sum_set, const float* grad_sigma_feat,
                               const ngp_vm_set* cat_set, const float* grad_prod, void* scratch, size_t scratch_bytes,
                               float* grads, void* stream) {
    const ngp_vm_set* sets[2] = {sum_set, cat_set};
    VmParams P;
    size_t total;
    const int rc = make_params("vm_backward", res0, res1, res2, sets, P, total);
    if (rc != NGP_OK) return rc;
    NGP_REQUIRE(sum_set || cat_set, NGP_ERR_ARG, "vm_backward: no set");
    NGP_REQUIRE((sum_set || !grad_sigma_feat) && (cat_set || !grad_prod), NGP_ERR_ARG,
                "vm_backward: a gradient without its set");
    NGP_REQUIRE(N <= (1u << 22), NGP_ERR_ARG, "vm_backward: N (%u) must be at most 2^22", N);
    const size_t need = kHdrWords * sizeof(uint32_t) + total * sizeof(fixed_t);
    NGP_REQUIRE(scratch && scratch_bytes >= need, NGP_ERR_ARG, "vm_backward: scratch of %zu bytes, %zu needed",
                scratch_bytes, need);
    NGP_REQUIRE(grads, NGP_ERR_ARG, "vm_backward: null gradient buffer");
    hipStream_t st = ngp_stream(stream);
    uint32_t* hdr = static_cast<uint32_t*>(scratch);
    fixed_t* acc = reinterpret_cast<fixed_t*>(hdr + kHdrWords);
    if (hipMemsetAsync(scratch, 0, need, st) != hipSuccess)
        return ngp_set_error(NGP_ERR_HIP, "vm_backward: hipMemsetAsync failed");
    uint32_t jobs = 0;
    uint32_t lds_rows = 0;
    for (int s = 0; s < 2; ++s) {
        if (!(s == 0 ? grad_sigma_feat : grad_prod)) continue;
        for (int i = 0; i < 3; ++i) {
            jobs += ngp_div_up(P.rank[s][i], kGroup);
            if (P.res[2 - i] <= kLdsLine && P.res[2 - i] > lds_rows) lds_rows = P.res[2 - i];
        }
    }
    if (N > 0 && jobs > 0) {
        NGP_REQUIRE(x && aabb6, NGP_ERR_ARG, "vm_backward: null buffer");
        const size_t na = grad_sigma_feat ? (size_t)N : 0, nb = grad_prod ? (size_t)N * P.width[1] : 0;
        const size_t most = (na > nb ? na : nb);
        const uint32_t gblocks = (uint32_t)(most / kThreads + 1 < 1024 ? most / kThreads + 1 : 1024);
        k_vm_gmax<<<gblocks, kThreads, 0, st>>>(grad_sigma_feat, na, grad_prod, nb, hdr);
        int rl = ngp_check_launch("vm_backward (max)");
        if (rl != NGP_OK) return rl;
        const dim3 grid(ngp_div_up(N, kChunkPoints), jobs);
        k_vm_backward<<<grid, kThreads, (size_t)lds_rows * kGroup * sizeof(fixed_t), st>>>(
            P, x, N, aabb6, grad_sigma_feat, grad_prod, hdr, acc);
        rl = ngp_check_launch("vm_backward");
        if (rl != NGP_OK) return rl;
    }
    const size_t fb = total / kThreads + 1;
    k_vm_finish<<<(uint32_t)(fb < 2048 ? fb : 2048), kThreads, 0, st>>>(acc, hdr, total, grads);
    return ngp_check_launch("vm_backward (finish)");
}
