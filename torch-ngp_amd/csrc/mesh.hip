// Triangle mesh of a density volume on the device: marching cubes over a
// lattice (reference nerf/utils.py extract_fields / extract_geometry :172-202
// and Trainer.save_mesh :688-708, which hand a host numpy volume to PyMCubes).
// DESIGN.md §11 has the conventions; the case table is generated
// (tools/gen_mc_table.py -> mc_table.h).
//
//   lattice index p = (i * ny + j) * nz + k (meshgrid 'ij', z fastest); a cell
//   is named by its minimum corner; a corner is inside when value >= threshold
//   (NaN: outside, read as 0 by the interpolation).
//
//   k_mesh_lattice      world positions of lattice points [lo, hi)
//   k_mesh_count        per point: which of its +x/+y/+z edges are crossed (3
//                       bits) and its cell's triangle count; per-block sums
//   k_mesh_scan_blocks  one workgroup: exclusive scan of the block sums in 64
//                       bits, totals V, T
//   k_mesh_prefix       per point: vert_prefix, tri_prefix (block scan + offset)
//   k_mesh_emit         vertices by (p, axis), triangles by (cell, table
//                       order), optional normals
//
// No atomics anywhere: every count comes from a scan, every output slot has
// one writer, so two runs give the same bytes. A block is 256 consecutive
// lattice points; its 8-corner reads are 4 streams of 257 consecutive values
// (p, p + nz, p + ny nz, p + ny nz + nz, each with the +1 point in z), staged
// in LDS so that the z neighbours are shared; the y / x neighbour rows are
// re-read by the blocks that own them and come from L2.
#define NGP_MC_TABLE_ATTR __device__
#include "ngp_common.h"

#include <cmath>

#include "mc_table.h"

namespace {

constexpr uint32_t kT = 256;          // lattice points per block
constexpr uint32_t kScanThreads = 1024;

struct MeshDims {
    uint32_t nx, ny, nz, N;
};

struct MeshBox {  // world = mn + ext * (lattice / den); unit: lattice units
    float mn[3], ext[3], den[3];
    int32_t world;
};

NGP_DEV float nan0(float v) { return v != v ? 0.0f : v; }

// the 4 corner streams of the block's points: s[2 x + y][t + z] is the corner
// (x, y, z) of the cell at p0 + t. Points past the volume read as 0; the
// resolution guards decide whether a neighbour exists before its value counts.
NGP_DEV void stage_corners(const float* __restrict__ vol, MeshDims d, uint32_t p0, float (*s)[kT + 1]) {
    const uint32_t t = threadIdx.x;
    const uint64_t row = d.nz, plane = (uint64_t)d.ny * d.nz;
#pragma unroll
    for (uint32_t r = 0; r < 4; ++r) {
        const uint64_t base = (uint64_t)p0 + (r >> 1) * plane + (r & 1) * row;
        const uint64_t q = base + t;
        s[r][t] = q < d.N ? vol[q] : 0.0f;
        if (t == r) s[r][kT] = base + kT < d.N ? vol[base + kT] : 0.0f;
    }
}

NGP_DEV void point_ijk(MeshDims d, uint32_t p, uint32_t& i, uint32_t& j, uint32_t& k) {
    const uint32_t q = p / d.nz;
    k = p - q * d.nz;
    i = q / d.ny;
    j = q - i * d.ny;
}

NGP_DEV uint32_t cell_case(const float (*s)[kT + 1], uint32_t t, float thr) {
    uint32_t c = 0;
#pragma unroll
    for (uint32_t corner = 0; corner < 8; ++corner) {
        const uint32_t x = corner & 1, y = corner >> 1 & 1, z = corner >> 2;
        c |= (uint32_t)(s[2 * x + y][t + z] >= thr) << corner;
    }
    return c;
}

__global__ void __launch_bounds__(kT) k_mesh_lattice(MeshDims d, MeshBox box, uint32_t lo, uint32_t hi,
                                                    float* __restrict__ xyzs) {
    const uint32_t q = lo + blockIdx.x * kT + threadIdx.x;
    if (q >= hi) return;
    uint32_t i, j, k;
    point_ijk(d, q, i, j, k);
    const uint32_t c[3] = {i, j, k};
    float* o = xyzs + (size_t)(q - lo) * 3;
#pragma unroll
    for (int a = 0; a < 3; ++a) o[a] = box.mn[a] + box.ext[a] * ((float)c[a] / box.den[a]);
}

// block sum of two small counts packed as lo | hi << 16 (each <= 5 per thread)
NGP_DEV uint32_t block_sum_packed(uint32_t v, uint32_t* red) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) red[wave] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

__global__ void __launch_bounds__(kT) k_mesh_count(const float* __restrict__ vol, MeshDims d, float thr,
                                                  uint8_t* __restrict__ flags, uint8_t* __restrict__ tcnt,
                                                  uint32_t* __restrict__ bsum) {
    __shared__ float s[4][kT + 1];
    __shared__ uint8_t ntri[256];
    __shared__ uint32_t red[kT / 64];
    const uint32_t t = threadIdx.x, p0 = blockIdx.x * kT, p = p0 + t;
    stage_corners(vol, d, p0, s);
    ntri[t] = kMcTriCount[t];
    __syncthreads();
    uint32_t f = 0, nt = 0;
    if (p < d.N) {
        uint32_t i, j, k;
        point_ijk(d, p, i, j, k);
        const bool in0 = s[0][t] >= thr;
        const bool ex = i + 1 < d.nx, ey = j + 1 < d.ny, ez = k + 1 < d.nz;
        f = (uint32_t)(ex && in0 != (s[2][t] >= thr)) | (uint32_t)(ey && in0 != (s[1][t] >= thr)) << 1 |
            (uint32_t)(ez && in0 != (s[0][t + 1] >= thr)) << 2;
        if (ex && ey && ez) nt = ntri[cell_case(s, t, thr)];
        flags[p] = (uint8_t)f;
        tcnt[p] = (uint8_t)nt;
    }
    const uint32_t sum = block_sum_packed((uint32_t)__popc(f) | nt << 16, red);
    if (t == 0) {
        bsum[2 * blockIdx.x] = sum & 0xffffu;
        bsum[2 * blockIdx.x + 1] = sum >> 16;
    }
}

// One workgroup: thread i sums a contiguous run of blocks, the 1024 run sums
// are scanned in LDS (Hillis-Steele, 64-bit), then each run is walked again.
__global__ void __launch_bounds__(kScanThreads) k_mesh_scan_blocks(const uint32_t* __restrict__ bsum, uint32_t nb,
                                                                  uint64_t* __restrict__ boff,
                                                                  uint64_t* __restrict__ counts) {
    __shared__ uint64_t sv[2][kScanThreads], st[2][kScanThreads];
    const uint32_t t = threadIdx.x;
    const uint32_t per = (nb + kScanThreads - 1) / kScanThreads;
    const uint64_t lo = (uint64_t)t * per;
    const uint64_t hi = lo + per < nb ? lo + per : nb;
    uint64_t v = 0, c = 0;
    for (uint64_t b = lo; b < hi; ++b) {
        v += bsum[2 * b];
        c += bsum[2 * b + 1];
    }
    int cur = 0;
    sv[0][t] = v;
    st[0][t] = c;
    __syncthreads();
    for (uint32_t off = 1; off < kScanThreads; off <<= 1) {
        const uint64_t a = sv[cur][t] + (t >= off ? sv[cur][t - off] : 0);
        const uint64_t b = st[cur][t] + (t >= off ? st[cur][t - off] : 0);
        sv[cur ^ 1][t] = a;
        st[cur ^ 1][t] = b;
        cur ^= 1;
        __syncthreads();
    }
    uint64_t ov = sv[cur][t] - v, oc = st[cur][t] - c;  // exclusive
    for (uint64_t b = lo; b < hi; ++b) {
        boff[2 * b] = ov;
        boff[2 * b + 1] = oc;
        ov += bsum[2 * b];
        oc += bsum[2 * b + 1];
    }
    if (t == kScanThreads - 1) {
        counts[0] = sv[cur][t];
        counts[1] = st[cur][t];
    }
}

__global__ void __launch_bounds__(kT) k_mesh_prefix(const uint8_t* __restrict__ flags,
                                                   const uint8_t* __restrict__ tcnt, uint32_t N,
                                                   const uint64_t* __restrict__ boff, uint32_t* __restrict__ vpre,
                                                   uint32_t* __restrict__ tpre) {
    __shared__ uint32_t wsum[kT / 64];
    const uint32_t t = threadIdx.x, p = blockIdx.x * kT + t, lane = t & 63, wave = t >> 6;
    const uint32_t mine = p < N ? (uint32_t)__popc((uint32_t)flags[p]) | (uint32_t)tcnt[p] << 16 : 0u;
    uint32_t inc = mine;  // inclusive scan in the wave; the packed halves cannot carry (<= 1280 per block)
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t up = __shfl_up(inc, off, 64);
        if (lane >= (uint32_t)off) inc += up;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    uint32_t before = 0;
    for (uint32_t w = 0; w < wave; ++w) before += wsum[w];
    const uint32_t exc = before + inc - mine;
    if (p < N) {
        // emit takes these only when V, T < 2^31 (ngp_mesh_emit), so 32 bits hold them
        vpre[p] = (uint32_t)(boff[2 * blockIdx.x] + (exc & 0xffffu));
        tpre[p] = (uint32_t)(boff[2 * blockIdx.x + 1] + (exc >> 16));
    }
}

NGP_DEV float vol_at(const float* __restrict__ vol, MeshDims d, int32_t i, int32_t j, int32_t k) {
    return nan0(vol[((size_t)i * d.ny + j) * d.nz + k]);
}

// the volume's gradient at a lattice point: central differences, one-sided on the border
NGP_DEV void point_gradient(const float* __restrict__ vol, MeshDims d, MeshBox box, const uint32_t c[3], float g[3]) {
    const uint32_t n[3] = {d.nx, d.ny, d.nz};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        int32_t lo[3] = {(int32_t)c[0], (int32_t)c[1], (int32_t)c[2]};
        int32_t hi[3] = {(int32_t)c[0], (int32_t)c[1], (int32_t)c[2]};
        if (c[a] > 0) lo[a] -= 1;
        if (c[a] + 1 < n[a]) hi[a] += 1;
        const float steps = (float)(hi[a] - lo[a]);  // 2 inside, 1 on the border
        float h = steps;
        if (box.world) h = steps * (box.ext[a] / box.den[a]);
        g[a] = (vol_at(vol, d, hi[0], hi[1], hi[2]) - vol_at(vol, d, lo[0], lo[1], lo[2])) / h;
    }
}

template <bool NORMALS>
__global__ void __launch_bounds__(kT) k_mesh_emit(const float* __restrict__ vol, MeshDims d, float thr, MeshBox box,
                                                 const uint8_t* __restrict__ flags,
                                                 const uint32_t* __restrict__ vpre,
                                                 const uint32_t* __restrict__ tpre, uint32_t V, uint32_t T,
                                                 float* __restrict__ vertices, float* __restrict__ normals,
                                                 int32_t* __restrict__ faces) {
    __shared__ float s[4][kT + 1];
    __shared__ int32_t tris[256 * 16 / 4];
    const uint32_t t = threadIdx.x, p0 = blockIdx.x * kT, p = p0 + t;
    stage_corners(vol, d, p0, s);
    {
        const int32_t* src = reinterpret_cast<const int32_t*>(&kMcTris[0][0]);
#pragma unroll
        for (uint32_t w = 0; w < 4; ++w) tris[w * kT + t] = src[w * kT + t];
    }
    __syncthreads();
    if (p >= d.N) return;
    uint32_t c[3];
    point_ijk(d, p, c[0], c[1], c[2]);
    const uint32_t f = flags[p];

    if (f) {
        const uint32_t vbase = vpre[p];
        const float a = nan0(s[0][t]);
        const float nb[3] = {nan0(s[2][t]), nan0(s[1][t]), nan0(s[0][t + 1])};
        float g0[3];
        if (NORMALS) point_gradient(vol, d, box, c, g0);
#pragma unroll
        for (uint32_t ax = 0; ax < 3; ++ax) {
            if (!(f >> ax & 1)) continue;
            const float tt = (thr - a) / (nb[ax] - a);
            const size_t vid = (size_t)vbase + __popc(f & ((1u << ax) - 1));
            if (vid >= V) continue;  // a workspace counted from another volume: never write past the outputs
#pragma unroll
            for (uint32_t m = 0; m < 3; ++m) {
                const float q0 = (float)c[m], q1 = (float)(c[m] + (m == ax ? 1u : 0u));
                float pos = q0 + tt * (q1 - q0);
                if (box.world) pos = box.mn[m] + box.ext[m] * (pos / box.den[m]);
                vertices[vid * 3 + m] = pos;
            }
            if (NORMALS) {
                uint32_t c1[3] = {c[0], c[1], c[2]};
                c1[ax] += 1;
                float g1[3], nrm[3];
                point_gradient(vol, d, box, c1, g1);
#pragma unroll
                for (int m = 0; m < 3; ++m) nrm[m] = -(g0[m] + tt * (g1[m] - g0[m]));
                const float len = sqrtf(nrm[0] * nrm[0] + nrm[1] * nrm[1] + nrm[2] * nrm[2]);
#pragma unroll
                for (int m = 0; m < 3; ++m) normals[vid * 3 + m] = len > 0.0f ? nrm[m] / len : 0.0f;
            }
        }
    }

    if (c[0] + 1 < d.nx && c[1] + 1 < d.ny && c[2] + 1 < d.nz) {
        const uint32_t cs = cell_case(s, t, thr);
        if (cs != 0 && cs != 255) {
            const int8_t* row = reinterpret_cast<const int8_t*>(tris) + cs * 16;
            const uint32_t plane = d.ny * d.nz;
            const size_t out = (size_t)tpre[p] * 3;
            for (uint32_t n = 0; n < 3 * NGP_MC_MAX_TRIS && row[n] >= 0 && out + n < (size_t)T * 3; ++n) {
                const uint32_t e = (uint32_t)row[n], ax = e >> 2, r = e & 3;
                const uint32_t base = (r & ((1u << ax) - 1)) | (r >> ax) << (ax + 1);  // r-th corner with bit ax clear
                // the owner exists: the cell does, so every corner is inside the volume
                const uint32_t q = p + (base & 1) * plane + (base >> 1 & 1) * d.nz + (base >> 2);
                faces[out + n] = (int32_t)(vpre[q] + __popc((uint32_t)flags[q] & ((1u << ax) - 1)));
            }
        }
    }
}

// ---- host side -----------------------------------------------------------------

struct MeshWs {
    size_t flags, tcnt, vpre, tpre, bsum, boff, total;
    uint32_t nb;
};

size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

MeshWs mesh_ws(uint32_t N) {
    MeshWs w{};
    w.nb = ngp_div_up(N, kT);
    size_t at = 0;
    w.flags = at; at = align256(at + N);
    w.tcnt = at; at = align256(at + N);
    w.vpre = at; at = align256(at + (size_t)N * 4);
    w.tpre = at; at = align256(at + (size_t)N * 4);
    w.bsum = at; at = align256(at + (size_t)w.nb * 8);
    w.boff = at; at = align256(at + (size_t)w.nb * 16);
    w.total = at;
    return w;
}

// 0 when a resolution is below 2 or the lattice has 2^31 points or more
uint32_t mesh_points(uint32_t nx, uint32_t ny, uint32_t nz) {
    if (nx < 2 || ny < 2 || nz < 2) return 0;
    const uint64_t xy = (uint64_t)nx * ny;
    if (xy >= (1ull << 31)) return 0;
    const uint64_t n = xy * nz;
    return n >= (1ull << 31) ? 0u : (uint32_t)n;
}

int mesh_check_dims(const char* what, uint32_t nx, uint32_t ny, uint32_t nz) {
    NGP_REQUIRE(nx >= 2 && ny >= 2 && nz >= 2, NGP_ERR_ARG, "%s: resolution %u x %u x %u, every axis needs >= 2 points",
                what, nx, ny, nz);
    NGP_REQUIRE(mesh_points(nx, ny, nz) != 0, NGP_ERR_ARG, "%s: %u x %u x %u lattice points do not fit in 31 bits",
                what, nx, ny, nz);
    return NGP_OK;
}

int mesh_box(const char* what, const float* aabb, uint32_t nx, uint32_t ny, uint32_t nz, MeshBox* box) {
    const uint32_t n[3] = {nx, ny, nz};
    box->world = aabb != nullptr;
    for (int a = 0; a < 3; ++a) {
        box->den[a] = (float)(n[a] - 1);
        if (!aabb) {
            box->mn[a] = 0.0f;
            box->ext[a] = box->den[a];
            continue;
        }
        NGP_REQUIRE(std::isfinite(aabb[a]) && std::isfinite(aabb[a + 3]) && aabb[a + 3] > aabb[a], NGP_ERR_ARG,
                    "%s: aabb axis %d needs finite min < max, got [%g, %g]", what, a, (double)aabb[a],
                    (double)aabb[a + 3]);
        box->mn[a] = aabb[a];
        box->ext[a] = aabb[a + 3] - aabb[a];
    }
    return NGP_OK;
}

}  // namespace

extern "C" int ngp_mesh_lattice_points(uint32_t nx, uint32_t ny, uint32_t nz, const float* aabb, uint32_t lo,
                                       uint32_t hi, float* xyzs, void* stream) {
    if (int e = mesh_check_dims("mesh_lattice_points", nx, ny, nz)) return e;
    NGP_REQUIRE(aabb && xyzs, NGP_ERR_ARG, "mesh_lattice_points: null aabb / xyzs");
    MeshBox box;
    if (int e = mesh_box("mesh_lattice_points", aabb, nx, ny, nz, &box)) return e;
    const uint32_t N = mesh_points(nx, ny, nz);
    NGP_REQUIRE(lo <= hi && hi <= N, NGP_ERR_ARG, "mesh_lattice_points: points [%u, %u) of %u", lo, hi, N);
    if (lo == hi) return NGP_OK;
    k_mesh_lattice<<<ngp_div_up(hi - lo, kT), kT, 0, ngp_stream(stream)>>>(MeshDims{nx, ny, nz, N}, box, lo, hi, xyzs);
    return ngp_check_launch("mesh_lattice_points");
}

extern "C" size_t ngp_mesh_workspace_bytes(uint32_t nx, uint32_t ny, uint32_t nz) {
    const uint32_t N = mesh_points(nx, ny, nz);
    return N ? mesh_ws(N).total : 0;
}

extern "C" int ngp_mesh_count(const float* volume, uint32_t nx, uint32_t ny, uint32_t nz, float threshold, void* ws,
                              size_t ws_bytes, uint64_t* counts, void* stream) {
    if (int e = mesh_check_dims("mesh_count", nx, ny, nz)) return e;
    NGP_REQUIRE(volume && ws && counts, NGP_ERR_ARG, "mesh_count: null volume / workspace / counts");
    NGP_REQUIRE(std::isfinite(threshold), NGP_ERR_ARG, "mesh_count: threshold must be finite");
    const uint32_t N = mesh_points(nx, ny, nz);
    const MeshWs w = mesh_ws(N);
    NGP_REQUIRE(ws_bytes >= w.total, NGP_ERR_ARG, "mesh_count: workspace of %zu bytes, %zu needed", ws_bytes, w.total);
    hipStream_t st = ngp_stream(stream);
    uint8_t* b = static_cast<uint8_t*>(ws);
    const MeshDims d{nx, ny, nz, N};
    uint32_t* bsum = reinterpret_cast<uint32_t*>(b + w.bsum);
    uint64_t* boff = reinterpret_cast<uint64_t*>(b + w.boff);
    k_mesh_count<<<w.nb, kT, 0, st>>>(volume, d, threshold, b + w.flags, b + w.tcnt, bsum);
    k_mesh_scan_blocks<<<1, kScanThreads, 0, st>>>(bsum, w.nb, boff, counts);
    k_mesh_prefix<<<w.nb, kT, 0, st>>>(b + w.flags, b + w.tcnt, N, boff, reinterpret_cast<uint32_t*>(b + w.vpre),
                                       reinterpret_cast<uint32_t*>(b + w.tpre));
    return ngp_check_launch("mesh_count");
}

extern "C" int ngp_mesh_emit(const float* volume, uint32_t nx, uint32_t ny, uint32_t nz, float threshold,
                             const float* aabb, const void* ws, size_t ws_bytes, uint64_t V, uint64_t T,
                             float* vertices, float* normals, int32_t* faces, void* stream) {
    if (int e = mesh_check_dims("mesh_emit", nx, ny, nz)) return e;
    NGP_REQUIRE(volume && ws, NGP_ERR_ARG, "mesh_emit: null volume / workspace");
    NGP_REQUIRE(std::isfinite(threshold), NGP_ERR_ARG, "mesh_emit: threshold must be finite");
    MeshBox box;
    if (int e = mesh_box("mesh_emit", aabb, nx, ny, nz, &box)) return e;
    const uint32_t N = mesh_points(nx, ny, nz);
    const MeshWs w = mesh_ws(N);
    NGP_REQUIRE(ws_bytes >= w.total, NGP_ERR_ARG, "mesh_emit: workspace of %zu bytes, %zu needed", ws_bytes, w.total);
    NGP_REQUIRE(V < (1ull << 31) && T < (1ull << 31), NGP_ERR_UNSUPPORTED,
                "mesh_emit: %llu vertices / %llu triangles do not fit int32 indices", (unsigned long long)V,
                (unsigned long long)T);
    NGP_REQUIRE((V == 0 || vertices) && (T == 0 || faces), NGP_ERR_ARG, "mesh_emit: null vertices / faces");
    if (V == 0 && T == 0) return NGP_OK;
    const uint8_t* b = static_cast<const uint8_t*>(ws);
    const MeshDims d{nx, ny, nz, N};
    const uint32_t* vpre = reinterpret_cast<const uint32_t*>(b + w.vpre);
    const uint32_t* tpre = reinterpret_cast<const uint32_t*>(b + w.tpre);
    hipStream_t st = ngp_stream(stream);
    if (normals)
        k_mesh_emit<true><<<w.nb, kT, 0, st>>>(volume, d, threshold, box, b + w.flags, vpre, tpre, (uint32_t)V,
                                              (uint32_t)T, vertices, normals, faces);
    else
        k_mesh_emit<false><<<w.nb, kT, 0, st>>>(volume, d, threshold, box, b + w.flags, vpre, tpre, (uint32_t)V,
                                               (uint32_t)T, vertices, normals, faces);
    return ngp_check_launch("mesh_emit");
}
