// What mesh export does after marching cubes (mesh.hip): connected components
// of the indexed mesh, the keep rule with an order-preserving compaction, and
// the two small kernels around the colour query of the vertices. The reference
// has none of this (its save_mesh hands the arrays to trimesh unprocessed);
// DESIGN.md §20 has the conventions.
//
//   k_cc_init       parent[v] = v, comp_faces[v] = 0
//   k_cc_hook       per triangle: union of its two edges' trees (lock-free)
//   k_cc_compress   labels[v] = root of v (in place); per triangle one count on its root
//   k_clean_roots   per root: component count, rule count, the largest
//   k_clean_flag    per triangle: kept or not, marks its vertices, block sums
//   k_clean_vsum    per vertex block: kept vertices
//   k_clean_scan    one workgroup: exclusive scan of the block sums, totals
//   k_clean_prefix  per vertex / triangle: its output slot
//   k_clean_emit    kept vertices, normals, faces (remapped) in their order
//   k_color_dirs    d = -n / |n|
//   k_color_finish  rgb8 = q(sigmoid(logits[0..2]))
//
// The labelling uses integer atomics only and its result does not depend on
// their order: labels[v] is the smallest vertex index of v's component and
// comp_faces a sum of ones. The compaction places through scans, one writer
// per slot, so two runs give the same bytes. No kernel waits for another
// thread: there is no spin, ticket or grid barrier anywhere in this file.
#include "ngp_common.h"

#include <cmath>

namespace {

constexpr uint32_t kT = 256;
constexpr uint32_t kScanThreads = 1024;

// ---- connected components -------------------------------------------------------

NGP_DEV int32_t cc_load(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// The root of v's tree. parent[x] <= x always, and parent[x] == x only at a
// root, so the walk strictly decreases and ends after at most v steps whatever
// other threads do meanwhile.
NGP_DEV int32_t cc_find(const int32_t* parent, int32_t v) {
    int32_t p = cc_load(parent + v);
    while (p != v) {
        v = p;
        p = cc_load(parent + v);
    }
    return v;
}

// cc_find that also halves the path it walks (parent[v] = grandparent): the
// stored value is an ancestor of v, so it is < v and in v's tree, and a root
// is never written (only a v with parent[v] != v is, and such a v never
// becomes a root again).
NGP_DEV int32_t cc_find_halve(int32_t* parent, int32_t v) {
    int32_t p = cc_load(parent + v);
    while (p != v) {
        const int32_t g = cc_load(parent + p);
        if (g != p) __hip_atomic_store(parent + v, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        v = p;
        p = g;
    }
    return v;
}

// Invariant of the whole labelling: parent[x] <= x for every x, with equality
// exactly at the roots, so every chain strictly decreases and its root is the
// smallest index of the tree. A root changes only through the compare-and-swap
// below, from itself to a smaller index of the tree it joins; a link is never
// undone, so two vertices once in one tree stay in one. The loop is bounded
// without reference to any other thread: a failed swap returns hi's new parent,
// which is < hi, so hi + lo strictly decreases with every iteration and the
// loop ends after at most a + b of them. Nothing is waited for.
NGP_DEV void cc_hook(int32_t* parent, int32_t a, int32_t b) {
    int32_t ra = cc_find_halve(parent, a), rb = cc_find_halve(parent, b);
    while (ra != rb) {
        const int32_t hi = ra > rb ? ra : rb, lo = ra > rb ? rb : ra;
        const int32_t seen = atomicCAS(parent + hi, hi, lo);
        if (seen == hi) return;  // hi was a root and now hangs under lo
        ra = cc_find_halve(parent, seen);  // hi had been hooked meanwhile: seen < hi
        rb = lo;
    }
}

__global__ void __launch_bounds__(kT) k_cc_init(uint32_t V, int32_t* __restrict__ parent,
                                               int32_t* __restrict__ comp_faces) {
    const uint32_t v = blockIdx.x * kT + threadIdx.x;
    if (v >= V) return;
    parent[v] = (int32_t)v;
    comp_faces[v] = 0;
}

NGP_DEV bool face_valid(int32_t a, int32_t b, int32_t c, uint32_t V) {
    return (uint32_t)a < V && (uint32_t)b < V && (uint32_t)c < V;  // a negative index is >= 2^31 > V
}

__global__ void __launch_bounds__(kT) k_cc_hook(const int32_t* __restrict__ faces, uint32_t T, uint32_t V,
                                               int32_t* parent) {
    const uint32_t t = blockIdx.x * kT + threadIdx.x;
    if (t >= T) return;
    const int32_t a = faces[3 * (size_t)t], b = faces[3 * (size_t)t + 1], c = faces[3 * (size_t)t + 2];
    if (!face_valid(a, b, c, V)) return;
    cc_hook(parent, a, b);
    cc_hook(parent, b, c);
}

// Thread i labels vertex i and counts triangle i on its root. The trees live in
// labels and are final here (no hook runs in this launch); vertex i's entry is
// replaced by its root in place, which to a find of another thread passing
// through i is a compressed path to the same root. The counts of a wave are
// summed per distinct root first (a mesh in cell order has one or two per
// wave), then added with one integer atomic each.
__global__ void __launch_bounds__(kT) k_cc_compress(const int32_t* __restrict__ faces, uint32_t T, uint32_t V,
                                                   int32_t* parent, int32_t* __restrict__ comp_faces) {
    const uint32_t i = blockIdx.x * kT + threadIdx.x, lane = threadIdx.x & 63;
    if (i < V)
        __hip_atomic_store(parent + i, cc_find(parent, (int32_t)i), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    int32_t root = -1;
    if (i < T) {
        const int32_t a = faces[3 * (size_t)i], b = faces[3 * (size_t)i + 1], c = faces[3 * (size_t)i + 2];
        if (face_valid(a, b, c, V)) root = cc_find(parent, a);
    }
    bool mine = root >= 0;
    // wave-uniform loop: every pass retires all lanes of one root, at most 64 passes
    for (uint64_t pend = __ballot(mine); pend; pend = __ballot(mine)) {
        const uint32_t leader = (uint32_t)__ffsll((long long)pend) - 1u;
        const int32_t r0 = __shfl(root, (int)leader, 64);
        const bool same = mine && root == r0;
        const uint64_t m = __ballot(same);
        if (lane == leader) atomicAdd(comp_faces + r0, (int32_t)__popcll(m));
        if (same) mine = false;
    }
}

// ---- cleaning ---------------------------------------------------------------------

struct CleanHdr {  // 16 bytes at the head of the workspace, zeroed by the count entry
    unsigned long long best;    // max over roots of (comp_faces << 32) | ~label: most triangles, then smallest label
    unsigned long long counts;  // roots | (roots with comp_faces >= min_faces) << 32; each < 2^31, so no carry crosses
};

struct CleanWs {
    size_t hdr, vused, fkeep, vpre, tpre, bsum, boff, total;
    uint32_t nb;
};

size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

CleanWs clean_ws(uint32_t V, uint32_t T) {
    CleanWs w{};
    w.nb = ngp_div_up(V > T ? V : T, kT);
    size_t at = 0;
    w.hdr = at; at = align256(at + sizeof(CleanHdr));
    w.vused = at; at = align256(at + V);  // hdr and vused are cleared by one memset
    w.fkeep = at; at = align256(at + T);
    w.vpre = at; at = align256(at + (size_t)V * 4);
    w.tpre = at; at = align256(at + (size_t)T * 4);
    w.bsum = at; at = align256(at + (size_t)w.nb * 8);
    w.boff = at; at = align256(at + (size_t)w.nb * 16);
    w.total = at;
    return w;
}

NGP_DEV bool comp_kept(int32_t label, const int32_t* __restrict__ comp_faces, uint32_t min_faces, bool keep_largest,
                       unsigned long long best) {
    if ((uint32_t)comp_faces[label] < min_faces) return false;
    return !keep_largest || (uint32_t)label == ~(uint32_t)best;
}

__global__ void __launch_bounds__(kT) k_clean_roots(const int32_t* __restrict__ labels,
                                                   const int32_t* __restrict__ comp_faces, uint32_t V,
                                                   uint32_t min_faces, CleanHdr* hdr) {
    const uint32_t v = blockIdx.x * kT + threadIdx.x, lane = threadIdx.x & 63;
    const bool root = v < V && labels[v] == (int32_t)v;
    const uint32_t cnt = root ? (uint32_t)comp_faces[v] : 0u;
    unsigned long long key = root ? ((unsigned long long)cnt << 32 | (uint32_t)~v) : 0ull;  // a root's key is > 0
    const uint64_t roots = __ballot(root), ruled = __ballot(root && cnt >= min_faces);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_down(key, off, 64);
        key = o > key ? o : key;
    }
    // per block two atomics at most: thousands of roots would otherwise queue on the header's two words
    __shared__ unsigned long long wkey[kT / 64], wsum[kT / 64];
    if (lane == 0) {
        wkey[threadIdx.x >> 6] = key;
        wsum[threadIdx.x >> 6] = (unsigned long long)__popcll(roots) | (unsigned long long)__popcll(ruled) << 32;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long k = wkey[0], s = wsum[0];
#pragma unroll
        for (uint32_t w = 1; w < kT / 64; ++w) {
            k = wkey[w] > k ? wkey[w] : k;
            s += wsum[w];
        }
        if (s) {  // a block with a root
            atomicAdd(&hdr->counts, s);
            atomicMax(&hdr->best, k);
        }
    }
}

// sum of a 0 / 1 flag over the block
NGP_DEV uint32_t block_count(bool f, uint32_t* red) {
    const uint32_t wave = threadIdx.x >> 6;
    const uint64_t m = __ballot(f);
    if ((threadIdx.x & 63) == 0) red[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

__global__ void __launch_bounds__(kT) k_clean_flag(const int32_t* __restrict__ faces, uint32_t T, uint32_t V,
                                                  const int32_t* __restrict__ labels,
                                                  const int32_t* __restrict__ comp_faces, uint32_t min_faces,
                                                  uint32_t keep_largest, const CleanHdr* __restrict__ hdr,
                                                  uint8_t* __restrict__ fkeep, uint8_t* vused,
                                                  uint32_t* __restrict__ bsum) {
    __shared__ uint32_t red[kT / 64];
    const uint32_t t = blockIdx.x * kT + threadIdx.x;
    bool keep = false;
    if (t < T) {
        const int32_t a = faces[3 * (size_t)t], b = faces[3 * (size_t)t + 1], c = faces[3 * (size_t)t + 2];
        if (face_valid(a, b, c, V)) {
            const int32_t l = labels[a];  // labels that are no ngp_mesh_components output are not followed
            keep = (uint32_t)l < V && comp_kept(l, comp_faces, min_faces, keep_largest != 0, hdr->best);
        }
        fkeep[t] = (uint8_t)keep;
        if (keep) vused[a] = vused[b] = vused[c] = 1;  // every writer stores the same byte
    }
    const uint32_t sum = block_count(keep, red);
    if (threadIdx.x == 0) bsum[2 * blockIdx.x + 1] = sum;
}

__global__ void __launch_bounds__(kT) k_clean_vsum(const uint8_t* __restrict__ vused, uint32_t V,
                                                  uint32_t* __restrict__ bsum) {
    __shared__ uint32_t red[kT / 64];
    const uint32_t v = blockIdx.x * kT + threadIdx.x;
    const uint32_t sum = block_count(v < V && vused[v] != 0, red);
    if (threadIdx.x == 0) bsum[2 * blockIdx.x] = sum;
}

// k_mesh_scan_blocks' scan (mesh.hip) on this file's block sums: thread i sums
// a contiguous run of blocks, the 1024 run sums are scanned in LDS
// (Hillis-Steele, 64-bit), then each run is walked again. counts: V', T', the
// components and the components the rule keeps.
__global__ void __launch_bounds__(kScanThreads) k_clean_scan(const uint32_t* __restrict__ bsum, uint32_t nb,
                                                            uint64_t* __restrict__ boff,
                                                            const CleanHdr* __restrict__ hdr, uint32_t min_faces,
                                                            uint32_t keep_largest, uint64_t* __restrict__ counts) {
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
        const uint32_t ncomp = (uint32_t)hdr->counts, nrule = (uint32_t)(hdr->counts >> 32);
        counts[2] = ncomp;
        // the largest component exists when there is a root at all; it is kept when it passes min_faces too
        counts[3] = keep_largest ? (uint64_t)(ncomp != 0 && (uint32_t)(hdr->best >> 32) >= min_faces)
                                 : (uint64_t)nrule;
    }
}

// exclusive position of a 0 / 1 flag inside the block
NGP_DEV uint32_t block_exclusive(bool f, uint32_t* wsum) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t m = __ballot(f);
    if (lane == 0) wsum[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t before = 0;
    for (uint32_t w = 0; w < wave; ++w) before += wsum[w];
    return before + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
}

__global__ void __launch_bounds__(kT) k_clean_prefix(const uint8_t* __restrict__ vused,
                                                    const uint8_t* __restrict__ fkeep, uint32_t V, uint32_t T,
                                                    const uint64_t* __restrict__ boff, uint32_t* __restrict__ vpre,
                                                    uint32_t* __restrict__ tpre) {
    __shared__ uint32_t wv[kT / 64], wt[kT / 64];
    const uint32_t i = blockIdx.x * kT + threadIdx.x;
    const uint32_t ev = block_exclusive(i < V && vused[i] != 0, wv);
    const uint32_t et = block_exclusive(i < T && fkeep[i] != 0, wt);
    // the emit entry takes these only when V', T' < 2^31, so 32 bits hold them
    if (i < V) vpre[i] = (uint32_t)boff[2 * blockIdx.x] + ev;
    if (i < T) tpre[i] = (uint32_t)boff[2 * blockIdx.x + 1] + et;
}

__global__ void __launch_bounds__(kT) k_clean_emit(const float* __restrict__ vertices,
                                                  const float* __restrict__ normals,
                                                  const int32_t* __restrict__ faces, uint32_t V, uint32_t T,
                                                  const uint8_t* __restrict__ vused,
                                                  const uint8_t* __restrict__ fkeep,
                                                  const uint32_t* __restrict__ vpre,
                                                  const uint32_t* __restrict__ tpre, uint32_t V2, uint32_t T2,
                                                  float* __restrict__ vertices_out, float* __restrict__ normals_out,
                                                  int32_t* __restrict__ faces_out) {
    const uint32_t i = blockIdx.x * kT + threadIdx.x;
    if (i < V && vused[i]) {
        const size_t o = vpre[i];
        if (o < V2) {  // a workspace counted from another mesh: never write past the outputs
#pragma unroll
            for (int m = 0; m < 3; ++m) vertices_out[o * 3 + m] = vertices[(size_t)i * 3 + m];
            if (normals_out) {
#pragma unroll
                for (int m = 0; m < 3; ++m) normals_out[o * 3 + m] = normals[(size_t)i * 3 + m];
            }
        }
    }
    if (i < T && fkeep[i]) {
        const size_t o = tpre[i];
        if (o < T2) {
#pragma unroll
            for (int m = 0; m < 3; ++m) {
                const uint32_t q = (uint32_t)faces[(size_t)i * 3 + m];
                faces_out[o * 3 + m] = q < V ? (int32_t)vpre[q] : 0;  // a kept face's indices are in range
            }
        }
    }
}

// ---- vertex colours -----------------------------------------------------------------

__global__ void __launch_bounds__(kT) k_color_dirs(const float* __restrict__ normals, uint32_t n,
                                                  float* __restrict__ dirs) {
    const uint32_t i = blockIdx.x * kT + threadIdx.x;
    if (i >= n) return;
    const float x = normals[(size_t)i * 3], y = normals[(size_t)i * 3 + 1], z = normals[(size_t)i * 3 + 2];
    const float len = sqrtf(x * x + y * y + z * z);
    float d[3] = {0.0f, 0.0f, 1.0f};
    if (len > 0.0f && len < INFINITY) {  // false for a NaN too
        d[0] = -x / len;
        d[1] = -y / len;
        d[2] = -z / len;
    }
#pragma unroll
    for (int m = 0; m < 3; ++m) dirs[(size_t)i * 3 + m] = d[m];
}

// frame.hip's quantise: x clamped to [0, 1], times 255, truncated; non-finite: 0
NGP_DEV uint32_t quantise(float x) {
    if (!(fabsf(x) < INFINITY)) return 0u;
    return (uint32_t)(fminf(fmaxf(x, 0.0f), 1.0f) * 255.0f);
}

__global__ void __launch_bounds__(kT) k_color_finish(const ngp_half* __restrict__ in, uint32_t stride, uint32_t n,
                                                    uint32_t logits, uint8_t* __restrict__ rgb) {
    const uint32_t i = blockIdx.x * kT + threadIdx.x;
    if (i >= n) return;
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        float x = (float)in[(size_t)i * stride + m];
        if (logits) x = 1.0f / (1.0f + expf(-x));
        rgb[(size_t)i * 3 + m] = (uint8_t)quantise(x);
    }
}

int clean_check_sizes(const char* what, uint64_t V, uint64_t T) {
    NGP_REQUIRE(V < (1ull << 31) && T < (1ull << 31), NGP_ERR_UNSUPPORTED,
                "%s: %llu vertices / %llu triangles do not fit int32 indices", what, (unsigned long long)V,
                (unsigned long long)T);
    return NGP_OK;
}

}  // namespace

extern "C" int ngp_mesh_components(const int32_t* faces, uint64_t V, uint64_t T, int32_t* labels,
                                   int32_t* comp_faces, void* stream) {
    NGP_REQUIRE((T == 0 || faces) && (V == 0 || (labels && comp_faces)), NGP_ERR_ARG,
                "mesh_components: null faces / labels / comp_faces");
    if (int e = clean_check_sizes("mesh_components", V, T)) return e;
    if (V == 0) return NGP_OK;  // no vertex: nothing to label, and every face is out of range
    hipStream_t st = ngp_stream(stream);
    const uint32_t v = (uint32_t)V, t = (uint32_t)T;
    int32_t* parent = labels;  // the trees are built in labels; k_cc_compress replaces each entry by its root
    k_cc_init<<<ngp_div_up(v, kT), kT, 0, st>>>(v, parent, comp_faces);
    if (t == 0) return ngp_check_launch("mesh_components");  // parent[v] = v is the labelling
    k_cc_hook<<<ngp_div_up(t, kT), kT, 0, st>>>(faces, t, v, parent);
    k_cc_compress<<<ngp_div_up(v > t ? v : t, kT), kT, 0, st>>>(faces, t, v, parent, comp_faces);
    return ngp_check_launch("mesh_components");
}

extern "C" size_t ngp_mesh_clean_workspace_bytes(uint64_t V, uint64_t T) {
    if (V >= (1ull << 31) || T >= (1ull << 31)) return 0;
    return clean_ws((uint32_t)V, (uint32_t)T).total;
}

extern "C" int ngp_mesh_clean_count(const int32_t* faces, uint64_t V, uint64_t T, const int32_t* labels,
                                    const int32_t* comp_faces, uint32_t min_faces, int32_t keep_largest, void* ws,
                                    size_t ws_bytes, uint64_t* counts, void* stream) {
    NGP_REQUIRE((T == 0 || faces) && (V == 0 || (labels && comp_faces)) && ws && counts, NGP_ERR_ARG,
                "mesh_clean_count: null faces / labels / comp_faces / workspace / counts");
    if (int e = clean_check_sizes("mesh_clean_count", V, T)) return e;
    const uint32_t v = (uint32_t)V, t = (uint32_t)T;
    const CleanWs w = clean_ws(v, t);
    NGP_REQUIRE(ws_bytes >= w.total, NGP_ERR_ARG, "mesh_clean_count: workspace of %zu bytes, %zu needed", ws_bytes,
                w.total);
    hipStream_t st = ngp_stream(stream);
    uint8_t* b = static_cast<uint8_t*>(ws);
    CleanHdr* hdr = reinterpret_cast<CleanHdr*>(b + w.hdr);
    uint32_t* bsum = reinterpret_cast<uint32_t*>(b + w.bsum);
    uint64_t* boff = reinterpret_cast<uint64_t*>(b + w.boff);
    if (hipMemsetAsync(b + w.hdr, 0, w.fkeep - w.hdr, st) != hipSuccess)
        return ngp_set_error(NGP_ERR_HIP, "mesh_clean_count: memset failed");
    if (w.nb == 0) {  // no vertex and no triangle: the totals are the zeros just written
        if (hipMemsetAsync(counts, 0, 4 * sizeof(uint64_t), st) != hipSuccess)
            return ngp_set_error(NGP_ERR_HIP, "mesh_clean_count: memset failed");
        return NGP_OK;
    }
    if (v) k_clean_roots<<<ngp_div_up(v, kT), kT, 0, st>>>(labels, comp_faces, v, min_faces, hdr);
    k_clean_flag<<<w.nb, kT, 0, st>>>(faces, t, v, labels, comp_faces, min_faces, keep_largest != 0, hdr, b + w.fkeep,
                                      b + w.vused, bsum);
    k_clean_vsum<<<w.nb, kT, 0, st>>>(b + w.vused, v, bsum);
    k_clean_scan<<<1, kScanThreads, 0, st>>>(bsum, w.nb, boff, hdr, min_faces, keep_largest != 0, counts);
    k_clean_prefix<<<w.nb, kT, 0, st>>>(b + w.vused, b + w.fkeep, v, t, boff, reinterpret_cast<uint32_t*>(b + w.vpre),
                                        reinterpret_cast<uint32_t*>(b + w.tpre));
    return ngp_check_launch("mesh_clean_count");
}

extern "C" int ngp_mesh_clean_emit(const float* vertices, const float* normals, const int32_t* faces, uint64_t V,
                                   uint64_t T, const void* ws, size_t ws_bytes, uint64_t V2, uint64_t T2,
                                   float* vertices_out, float* normals_out, int32_t* faces_out, void* stream) {
    NGP_REQUIRE(ws && (V == 0 || vertices) && (T == 0 || faces), NGP_ERR_ARG,
                "mesh_clean_emit: null vertices / faces / workspace");
    NGP_REQUIRE(!normals_out || normals || V == 0, NGP_ERR_ARG, "mesh_clean_emit: normals_out without normals");
    if (int e = clean_check_sizes("mesh_clean_emit", V, T)) return e;
    NGP_REQUIRE(V2 <= V && T2 <= T, NGP_ERR_ARG, "mesh_clean_emit: %llu / %llu kept of %llu / %llu",
                (unsigned long long)V2, (unsigned long long)T2, (unsigned long long)V, (unsigned long long)T);
    NGP_REQUIRE((V2 == 0 || vertices_out) && (T2 == 0 || faces_out), NGP_ERR_ARG,
                "mesh_clean_emit: null vertices_out / faces_out");
    const uint32_t v = (uint32_t)V, t = (uint32_t)T;
    const CleanWs w = clean_ws(v, t);
    NGP_REQUIRE(ws_bytes >= w.total, NGP_ERR_ARG, "mesh_clean_emit: workspace of %zu bytes, %zu needed", ws_bytes,
                w.total);
    if (V2 == 0 && T2 == 0) return NGP_OK;
    const uint8_t* b = static_cast<const uint8_t*>(ws);
    k_clean_emit<<<w.nb, kT, 0, ngp_stream(stream)>>>(
        vertices, normals, faces, v, t, b + w.vused, b + w.fkeep, reinterpret_cast<const uint32_t*>(b + w.vpre),
        reinterpret_cast<const uint32_t*>(b + w.tpre), (uint32_t)V2, (uint32_t)T2, vertices_out, normals_out,
        faces_out);
    return ngp_check_launch("mesh_clean_emit");
}

extern "C" int ngp_mesh_color_dirs(const float* normals, uint64_t n, float* dirs, void* stream) {
    NGP_REQUIRE(n == 0 || (normals && dirs), NGP_ERR_ARG, "mesh_color_dirs: null normals / dirs");
    NGP_REQUIRE(n < (1ull << 31), NGP_ERR_UNSUPPORTED, "mesh_color_dirs: %llu rows", (unsigned long long)n);
    if (n == 0) return NGP_OK;
    k_color_dirs<<<ngp_div_up((uint32_t)n, kT), kT, 0, ngp_stream(stream)>>>(normals, (uint32_t)n, dirs);
    return ngp_check_launch("mesh_color_dirs");
}

extern "C" int ngp_mesh_color_finish(const void* values, uint32_t stride, uint64_t n, int32_t logits, uint8_t* rgb,
                                     void* stream) {
    NGP_REQUIRE(n == 0 || (values && rgb), NGP_ERR_ARG, "mesh_color_finish: null values / rgb");
    NGP_REQUIRE(stride >= 3, NGP_ERR_ARG, "mesh_color_finish: a row of %u values holds no rgb", stride);
    NGP_REQUIRE(n < (1ull << 31), NGP_ERR_UNSUPPORTED, "mesh_color_finish: %llu rows", (unsigned long long)n);
    if (n == 0) return NGP_OK;
    k_color_finish<<<ngp_div_up((uint32_t)n, kT), kT, 0, ngp_stream(stream)>>>(
        static_cast<const ngp_half*>(values), stride, (uint32_t)n, logits != 0, rgb);
    return ngp_check_launch("mesh_color_finish");
}
