// Signed distance fields of triangle meshes: the device side of main_sdf.py.
//
// The reference's sdf/provider.py draws its batch on the host (trimesh's
// area-weighted surface sampler, provider.py:66-75) and signs it with pysdf
// (:51, :75); loss.py's mape_loss is the criterion. Here
//
//   ngp_sdf_sample  draws the batch in the reference's layout from the
//                   project's counter RNG (ngp_head.h), one thread per point;
//   ngp_sdf_query   gives the exact signed distance to the prepared mesh: the
//                   minimum over all faces of the point-to-triangle distance
//                   (the seven-region test of Ericson, Real-Time Collision
//                   Detection 5.1.5), signed by the pseudo-normal of the
//                   closest feature (Baerentzen and Aanaes 2005);
//   ngp_sdf_mape    is the loss and its gradient in one pass, the sum in a
//                   fixed order.
//
// Plain C++ HIP, vector stores only. Every float operation below is written
// in the order tests/sdf_helpers.py restates in numpy float32 (the library is
// built with -ffp-contract=off). DESIGN.md 21.
#include "ngp_common.h"
#include "ngp_head.h"

#include <cfloat>

namespace {

using ngp_head::rng_u32;
using ngp_head::rng_unit;

constexpr uint32_t kBlockFaces = NGP_SDF_BLOCK_FACES;
constexpr uint32_t kQueryThreads = 64;  // one wave per workgroup: the cull's decision is the workgroup's
constexpr uint32_t kSampleThreads = 256;
constexpr uint32_t kMapeThreads = 256;
constexpr uint32_t kMapeBlocks = NGP_SDF_MAPE_BLOCKS;

NGP_DEV float dot3(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }

// Closest point of triangle t = (a, b, c) to p: the squared distance, p - q
// and the feature q lies on (0 face, 1 2 3 the edges ab bc ca, 4 5 6 the
// vertices a b c). Ericson's regions in his order, without branches; one
// division. A vertex gives p - vertex itself, an edge (p - origin) - t * edge.
NGP_DEV void closest(float px, float py, float pz, const float* t, float& dist2, float& dx, float& dy, float& dz,
                     int& code) {
    const float ax = t[0], ay = t[1], az = t[2], bx = t[3], by = t[4], bz = t[5], cx = t[6], cy = t[7], cz = t[8];
    const float abx = bx - ax, aby = by - ay, abz = bz - az;
    const float acx = cx - ax, acy = cy - ay, acz = cz - az;
    const float bcx = cx - bx, bcy = cy - by, bcz = cz - bz;
    const float apx = px - ax, apy = py - ay, apz = pz - az;
    const float bpx = px - bx, bpy = py - by, bpz = pz - bz;
    const float cpx = px - cx, cpy = py - cy, cpz = pz - cz;
    const float d1 = dot3(abx, aby, abz, apx, apy, apz), d2 = dot3(acx, acy, acz, apx, apy, apz);
    const float d3 = dot3(abx, aby, abz, bpx, bpy, bpz), d4 = dot3(acx, acy, acz, bpx, bpy, bpz);
    const float d5 = dot3(abx, aby, abz, cpx, cpy, cpz), d6 = dot3(acx, acy, acz, cpx, cpy, cpz);
    const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    const float e43 = d4 - d3, e56 = d5 - d6;
    const bool isA = d1 <= 0.0f && d2 <= 0.0f;
    const bool isB = d3 >= 0.0f && d4 <= d3;
    const bool isAB = vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f;
    const bool isC = d6 >= 0.0f && d5 <= d6;
    const bool isCA = vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f;
    const bool isBC = va <= 0.0f && e43 >= 0.0f && e56 >= 0.0f;
    code = isA ? 4 : isB ? 5 : isAB ? 1 : isC ? 6 : isCA ? 3 : isBC ? 2 : 0;
    const float den = code == 1 ? d1 - d3 : code == 3 ? d2 - d6 : code == 2 ? e43 + e56 : code == 0 ? (va + vb) + vc : 1.0f;
    const float r = 1.0f / den;
    const float t1 = code == 1 ? d1 * r : code == 0 ? vb * r : 0.0f;                         // along ab
    const float t2 = code == 3 ? d2 * r : code == 2 ? e43 * r : code == 0 ? vc * r : 0.0f;   // along ac (bc for 2)
    const bool fromB = code == 5 || code == 2, fromC = code == 6;
    const float ox = fromB ? bpx : fromC ? cpx : apx, oy = fromB ? bpy : fromC ? cpy : apy,
                oz = fromB ? bpz : fromC ? cpz : apz;
    const float ex = code == 2 ? bcx : acx, ey = code == 2 ? bcy : acy, ez = code == 2 ? bcz : acz;
    dx = (ox - t1 * abx) - t2 * ex;
    dy = (oy - t1 * aby) - t2 * ey;
    dz = (oz - t1 * abz) - t2 * ez;
    dist2 = dot3(dx, dy, dz, dx, dy, dz);
}

// The squared distance past which nothing can replace a best of best2: a
// computed distance differs from the true one by the rounding of p - q, a few
// ulps of coordinates that prepare_mesh keeps below 2, under 1e-6, and a box
// distance likewise; 1e-5 relative and 1e-5 absolute cover both with room to
// spare. FLT_MAX (no best yet) gives +inf: nothing is past it.
NGP_DEV float cull_threshold(float best2) {
    const float t = sqrtf(best2) * 1.00001f + 1e-5f;
    return t * t;
}

// Squared distance from p to the box [lo, hi] (0 inside).
NGP_DEV float box_dist2(float px, float py, float pz, const float* lo, const float* hi) {
    const float qx = fmaxf(fmaxf(lo[0] - px, px - hi[0]), 0.0f);
    const float qy = fmaxf(fmaxf(lo[1] - py, py - hi[1]), 0.0f);
    const float qz = fmaxf(fmaxf(lo[2] - pz, pz - hi[2]), 0.0f);
    return dot3(qx, qy, qz, qx, qy, qz);
}

constexpr uint32_t kStage = 16;  // floats per staged face: its box (6), its corners (9), one of padding

// One thread per point, one wave per workgroup. The faces go through LDS a
// block of kBlockFaces at a time, each with its own box (every lane reads the
// same face: a broadcast). A smaller squared distance replaces the best one
// (strictly: ties keep the earlier face). A face whose box is past the lane's
// cull_threshold is not evaluated: it could not have replaced the best, so the
// result is that of evaluating every face. With cull, a block of faces is
// skipped when its box is past the threshold of every lane of the wave, and a
// lane's threshold starts from the smallest over the blocks of the distance to
// a box's farthest corner, which no nearest face can exceed; the results are
// the plain scan's bit for bit.
__global__ void __launch_bounds__(kQueryThreads)
k_sdf_query(const float* __restrict__ points, uint32_t n, const float* __restrict__ tris,
            const float* __restrict__ normals, const float* __restrict__ boxes, uint32_t T,
            const int32_t* __restrict__ tri, int cull, float* __restrict__ sdf, int32_t* __restrict__ feature) {
    __shared__ float stage[kBlockFaces * kStage];
    const uint32_t i = blockIdx.x * kQueryThreads + threadIdx.x;
    const bool live = i < n;
    const uint32_t ip = live ? i : n - 1;  // idle lanes of the last wave repeat its last point
    const float px = points[(size_t)ip * 3], py = points[(size_t)ip * 3 + 1], pz = points[(size_t)ip * 3 + 2];
    float best = FLT_MAX, bx = 0.0f, by = 0.0f, bz = 0.0f;
    int bface = 0, bcode = 0;
    if (tri) {
        const int32_t t0 = tri[ip];
        if (t0 >= 0 && (uint32_t)t0 < T) {
            closest(px, py, pz, tris + (size_t)t0 * 9, best, bx, by, bz, bcode);
            bface = t0;
            if (!(best == best)) best = FLT_MAX;  // a NaN start is no start
        }
    }
    const uint32_t nblocks = (T + kBlockFaces - 1) / kBlockFaces;
    float cap = INFINITY;  // the threshold of the blocks' upper bound
    if (cull) {
        float ub = FLT_MAX;
        for (uint32_t blk = 0; blk < nblocks; ++blk) {
            const float* bb = boxes + (size_t)blk * 6;
            const float fx = fmaxf(fabsf(px - bb[0]), fabsf(px - bb[3]));
            const float fy = fmaxf(fabsf(py - bb[1]), fabsf(py - bb[4]));
            const float fz = fmaxf(fabsf(pz - bb[2]), fabsf(pz - bb[5]));
            ub = fminf(ub, dot3(fx, fy, fz, fx, fy, fz));
        }
        cap = cull_threshold(ub);
    }
    float thr = fminf(cull_threshold(best), cap);
    for (uint32_t blk = 0; blk < nblocks; ++blk) {
        if (cull) {
            const float* bb = boxes + (size_t)blk * 6;
            if (__ballot(!(box_dist2(px, py, pz, bb, bb + 3) > thr)) == 0) continue;  // wave == workgroup: uniform
        }
        const uint32_t f0 = blk * kBlockFaces;
        const uint32_t cnt = min(kBlockFaces, T - f0);
        __syncthreads();
        if (threadIdx.x < cnt) {
            const float* src = tris + (size_t)(f0 + threadIdx.x) * 9;
            float* dst = stage + threadIdx.x * kStage;
            float v[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) v[k] = src[k];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                dst[k] = fminf(fminf(v[k], v[3 + k]), v[6 + k]);
                dst[3 + k] = fmaxf(fmaxf(v[k], v[3 + k]), v[6 + k]);
            }
#pragma unroll
            for (int k = 0; k < 9; ++k) dst[6 + k] = v[k];
        }
        __syncthreads();
        for (uint32_t f = 0; f < cnt; ++f) {
            const float* sf = stage + f * kStage;
            if (box_dist2(px, py, pz, sf, sf + 3) > thr) continue;
            float d, x, y, z;
            int c;
            closest(px, py, pz, sf + 6, d, x, y, z, c);
            if (d < best) {
                best = d; bx = x; by = y; bz = z;
                bface = (int)(f0 + f); bcode = c;
                thr = fminf(cull_threshold(best), cap);
            }
        }
    }
    if (!live) return;
    const float* nf = normals + ((size_t)bface * 7 + bcode) * 3;
    const float s = dot3(bx, by, bz, nf[0], nf[1], nf[2]);
    const float d = sqrtf(best);
    sdf[i] = s < 0.0f ? -d : d;
    if (feature) feature[i] = bface * 8 + bcode;
}

// One thread per point. counter[0] is the step every thread reads; the last
// workgroup to finish (a ticket in counter[1]) advances it and clears the
// ticket, so the next launch on the stream finds step + 1.
__global__ void __launch_bounds__(kSampleThreads)
k_sdf_sample(const float* __restrict__ tris, const float* __restrict__ cdf, uint32_t T, uint32_t N, uint32_t seed,
             uint32_t* counter, float* __restrict__ points, int32_t* __restrict__ tri_out) {
    const uint32_t step = __atomic_load_n(counter, __ATOMIC_RELAXED);
    const uint32_t i = blockIdx.x * kSampleThreads + threadIdx.x;
    if (i < N) {
        float x, y, z;
        int32_t t = -1;
        if (i < N / 8 * 7) {
            const float u0 = rng_unit(seed, step, i, 0);
            uint32_t lo = 0, hi = T - 1;
            while (lo < hi) {  // the first triangle whose cumulative area exceeds u0
                const uint32_t mid = (lo + hi) >> 1;
                if (u0 < cdf[mid]) hi = mid; else lo = mid + 1;
            }
            t = (int32_t)lo;
            const float* v = tris + (size_t)lo * 9;
            const float su = sqrtf(rng_unit(seed, step, i, 1)), u2 = rng_unit(seed, step, i, 2);
            const float b0 = 1.0f - su, b1 = su * (1.0f - u2), b2 = su * u2;
            x = (b0 * v[0] + b1 * v[3]) + b2 * v[6];
            y = (b0 * v[1] + b1 * v[4]) + b2 * v[7];
            z = (b0 * v[2] + b1 * v[5]) + b2 * v[8];
            if (i >= N / 2) {
                // Box-Muller: two pairs for three normals; the radius takes (k + 1) * 2^-24 in (0, 1]
                const float ua = (float)((rng_u32(seed, step, i, 3) >> 8) + 1u) * (1.0f / 16777216.0f);
                const float ub = rng_unit(seed, step, i, 4);
                const float uc = (float)((rng_u32(seed, step, i, 5) >> 8) + 1u) * (1.0f / 16777216.0f);
                const float ud = rng_unit(seed, step, i, 6);
                const float ra = sqrtf(-2.0f * logf(ua)), rc = sqrtf(-2.0f * logf(uc));
                const float pa = 6.2831855f * ub, pc = 6.2831855f * ud;
                x = x + 0.01f * (ra * cosf(pa));
                y = y + 0.01f * (ra * sinf(pa));
                z = z + 0.01f * (rc * cosf(pc));
            }
        } else {
            x = rng_unit(seed, step, i, 0) * 2.0f - 1.0f;
            y = rng_unit(seed, step, i, 1) * 2.0f - 1.0f;
            z = rng_unit(seed, step, i, 2) * 2.0f - 1.0f;
        }
        points[(size_t)i * 3] = x;
        points[(size_t)i * 3 + 1] = y;
        points[(size_t)i * 3 + 2] = z;
        if (tri_out) tri_out[i] = t;
    }
    __syncthreads();  // every thread of the workgroup has read the step
    if (threadIdx.x == 0) {
        const uint32_t ticket = atomicAdd(counter + 1, 1u);
        if (ticket == gridDim.x - 1) {
            __atomic_store_n(counter + 1, 0u, __ATOMIC_RELAXED);
            __atomic_store_n(counter, step + 1u, __ATOMIC_RELAXED);
        }
    }
}

NGP_DEV void put(float* p, float v) { *p = v; }
NGP_DEV void put(ngp_half* p, float v) { *p = ngp_f2h(v); }

NGP_DEV double block_sum(double v, double* sh) {
    sh[threadIdx.x] = v;
    __syncthreads();
    for (uint32_t s = kMapeThreads / 2; s > 0; s >>= 1) {
        if (threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
        __syncthreads();
    }
    return sh[0];
}

// Workgroup b takes elements [b * chunk, (b + 1) * chunk): thread t adds its
// elements t, t + 256, ... in order, then the tree above.
template <typename T>
__global__ void __launch_bounds__(kMapeThreads)
k_sdf_mape(const T* __restrict__ pred, const float* __restrict__ y, uint64_t n, uint64_t chunk,
           const float* __restrict__ grad_scale, T* __restrict__ grad, double* __restrict__ partials) {
    __shared__ double sh[kMapeThreads];
    const uint64_t lo = (uint64_t)blockIdx.x * chunk;
    const uint64_t hi = lo + chunk < n ? lo + chunk : n;
    const float inv_n = 1.0f / (float)n;
    const float scale = grad_scale ? *grad_scale : 1.0f;
    double acc = 0.0;
    for (uint64_t i = lo + threadIdx.x; i < hi; i += kMapeThreads) {
        const float p = (float)pred[i], t = y[i];
        acc += fabs((double)p - (double)t) / (fabs((double)t) + 1e-2);
        if (grad) {
            // torch's backward of mean(|p - t| / (|t| + 0.01)) in fp32: (1 / n) / (|t| + 0.01f) * sign(p - t)
            const float diff = p - t;
            const float sg = diff > 0.0f ? 1.0f : diff < 0.0f ? -1.0f : 0.0f;
            float g = (inv_n / (fabsf(t) + 0.01f)) * sg;
            if (grad_scale) g = g * scale;
            put(grad + i, g);
        }
    }
    const double s = block_sum(acc, sh);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

__global__ void __launch_bounds__(kMapeThreads)
k_sdf_mape_finish(const double* __restrict__ partials, uint32_t nparts, uint64_t n, double* __restrict__ loss) {
    __shared__ double sh[kMapeThreads];
    const double s = block_sum(threadIdx.x < nparts ? partials[threadIdx.x] : 0.0, sh);
    if (threadIdx.x == 0) *loss = s / (double)n;
}

}  // namespace

extern "C" int ngp_sdf_sample(const float* tris, const float* cdf, uint32_t T, uint32_t N, uint32_t seed,
                              uint32_t* counter, float* points, int32_t* tri, void* stream) {
    NGP_REQUIRE(N % 8 == 0, NGP_ERR_ARG, "sdf_sample: N (%u) must be divisible by 8", N);
    if (N == 0) return NGP_OK;
    NGP_REQUIRE(T >= 1 && T < (1u << 28), NGP_ERR_ARG, "sdf_sample: T (%u) must be in [1, 2^28)", T);
    NGP_REQUIRE(N < (1u << 30), NGP_ERR_ARG, "sdf_sample: N (%u) must be below 2^30", N);
    NGP_REQUIRE(tris && cdf && counter && points, NGP_ERR_ARG, "sdf_sample: null buffer");
    k_sdf_sample<<<ngp_div_up(N, kSampleThreads), kSampleThreads, 0, ngp_stream(stream)>>>(tris, cdf, T, N, seed,
                                                                                            counter, points, tri);
    return ngp_check_launch("sdf_sample");
}

extern "C" int ngp_sdf_query(const float* points, uint32_t n, const float* tris, const float* normals,
                             const float* block_aabb, uint32_t T, const int32_t* tri, int32_t cull, float* sdf,
                             int32_t* feature, void* stream) {
    if (n == 0) return NGP_OK;
    NGP_REQUIRE(T >= 1 && T < (1u << 28), NGP_ERR_ARG, "sdf_query: T (%u) must be in [1, 2^28)", T);
    NGP_REQUIRE(n < (1u << 30), NGP_ERR_ARG, "sdf_query: n (%u) must be below 2^30", n);
    NGP_REQUIRE(points && tris && normals && sdf, NGP_ERR_ARG, "sdf_query: null buffer");
    NGP_REQUIRE(!cull || block_aabb, NGP_ERR_ARG, "sdf_query: cull needs the block boxes");
    k_sdf_query<<<ngp_div_up(n, kQueryThreads), kQueryThreads, 0, ngp_stream(stream)>>>(
        points, n, tris, normals, block_aabb, T, tri, cull ? 1 : 0, sdf, feature);
    return ngp_check_launch("sdf_query");
}

extern "C" int ngp_sdf_mape(const void* pred, int32_t pred_dtype, const float* y, uint64_t n,
                            const float* grad_scale, void* grad, double* partials, double* loss, void* stream) {
    NGP_REQUIRE(pred_dtype == NGP_DTYPE_F32 || pred_dtype == NGP_DTYPE_F16, NGP_ERR_ARG,
                "sdf_mape: pred must be fp32 or fp16");
    NGP_REQUIRE(n >= 1 && n < (1ull << 24), NGP_ERR_ARG, "sdf_mape: n must be in [1, 2^24)");
    NGP_REQUIRE(pred && y && partials && loss, NGP_ERR_ARG, "sdf_mape: null buffer");
    uint64_t parts = (n + kMapeThreads - 1) / kMapeThreads;
    if (parts > kMapeBlocks) parts = kMapeBlocks;
    const uint64_t chunk = (n + parts - 1) / parts;
    parts = (n + chunk - 1) / chunk;
    hipStream_t s = ngp_stream(stream);
    if (pred_dtype == NGP_DTYPE_F32)
        k_sdf_mape<float><<<(uint32_t)parts, kMapeThreads, 0, s>>>((const float*)pred, y, n, chunk, grad_scale,
                                                                   (float*)grad, partials);
    else
        k_sdf_mape<ngp_half><<<(uint32_t)parts, kMapeThreads, 0, s>>>((const ngp_half*)pred, y, n, chunk, grad_scale,
                                                                      (ngp_half*)grad, partials);
    k_sdf_mape_finish<<<1, kMapeThreads, 0, s>>>(partials, (uint32_t)parts, n, loss);
    return ngp_check_launch("sdf_mape");
}
