// Baseline JPEG (ITU-T T.81, SOF0, 8 bit, JFIF) of a uint8 image on the device:
// the entropy-coded scan of a finished frame (FrameRenderer.rgb8 / depth8), so
// a test render can be kept as Motion-JPEG without the pixels crossing to the
// host. nerf/jpeg.py writes the header segments and EOI around the scan;
// nerf/video.py puts the files into an AVI. DESIGN.md §19.
//
// 3 components (Y, Cb, Cr, all 1 x 1: 4:4:4) or 1; an MCU is one 8 x 8 block per
// component. The restart interval is one MCU row, so every row of blocks is a
// byte-aligned stream of its own with its own DC predictors, and a wave can code
// it without knowing the rows above. Three launches per image:
//
//   k_jpeg_transform  a wave per MCU, a lane per pixel: JFIF colour conversion,
//                     level shift, the 8 x 8 DCT-II (row pass and column pass
//                     through LDS, fp32, each sum in index order), division by
//                     the quantiser, round to nearest, clamp, zigzag -> the int16
//                     workspace [blocks, 64] in MCU order
//   k_jpeg_code       a wave per restart interval, a lane per block, 64 blocks
//                     at a time: each lane measures its block's bits, a wave
//                     prefix sum gives its bit offset, each lane writes its codes
//                     at that offset into one LDS bit buffer (integer OR, so two
//                     lanes meeting in a word do not depend on order), then the
//                     wave byte-stuffs the buffer (ballot + prefix count) into
//                     the interval's slab; bits short of a byte are carried into
//                     the next 64 blocks, the last byte is padded with ones
//   k_jpeg_compact    a workgroup per interval: the slabs' lengths summed in
//                     index order give its offset; slab and RSTm into the output
//
// Sizes (ngp_jpeg_scan_capacity). The coder emits, per block, one code and its
// magnitude bits per nonzero coefficient, one ZRL per 16 zeros before a nonzero
// coefficient and one EOB when the block ends in zeros. Charge each ZRL to the
// first of its 16 zeros and the EOB to the first trailing zero: every one of the
// 64 coefficients then pays for at most one code (at most 16 bits, the longest
// a Huffman code of T.81 can be) and at most 11 magnitude bits (the largest DC
// difference category of baseline; AC has at most 10), 27 bits. A block is at
// most 64 * 27 = 1728 bits = 216 bytes; an interval of B blocks at most 216 B
// bytes of data plus at most one byte that the padding completes; byte stuffing
// at most doubles that: 2 (216 B + 1) bytes, the slab's size. With the 2 bytes
// of RSTm after each interval (the last has none: slack), the scan of n
// intervals is at most n * (2 (216 B + 1) + 2) bytes.
#include "ngp_common.h"
#include "jpeg_tables.h"

#include <cmath>

namespace {

constexpr uint32_t kCoefBits = 27;                 // 16-bit code + 11 magnitude bits
constexpr uint32_t kBlockBytes = 64 * kCoefBits / 8;  // 216
constexpr uint32_t kWave = 64;
// the bit buffer of 64 blocks: 7 carried bits + 64 * 1728, and one word past the last for a code's low half
constexpr uint32_t kBitWords = (7 + kWave * 64 * kCoefBits + 31) / 32 + 2;
constexpr uint32_t kCoefStride = 33;  // dwords per block in LDS: 32 + 1, lanes on distinct banks

struct Layout {
    uint32_t comps, mcus_x, mcus_y, n_mcus, bpi;  // bpi: blocks per interval
    uint64_t blocks;
    uint64_t slab_cap, slab_stride;   // bytes
    uint64_t len_off, slab_off;       // byte offsets into the workspace
    uint64_t ws_bytes, scan_cap;
};

Layout layout(uint32_t H, uint32_t W, uint32_t comps) {
    Layout l{};
    l.comps = comps;
    l.mcus_x = ngp_div_up(W, 8u);
    l.mcus_y = ngp_div_up(H, 8u);
    l.n_mcus = l.mcus_x * l.mcus_y;
    l.bpi = l.mcus_x * comps;
    l.blocks = (uint64_t)l.n_mcus * comps;
    l.slab_cap = 2ull * ((uint64_t)l.bpi * kBlockBytes + 1ull);
    l.slab_stride = (l.slab_cap + 15ull) & ~15ull;
    l.len_off = l.blocks * 128ull;  // a multiple of 16
    l.slab_off = l.len_off + (((uint64_t)l.mcus_y * 4ull + 15ull) & ~15ull);
    l.ws_bytes = l.slab_off + (uint64_t)l.mcus_y * l.slab_stride;
    l.scan_cap = (uint64_t)l.mcus_y * (l.slab_cap + 2ull);
    return l;
}

bool valid_shape(uint32_t H, uint32_t W, uint32_t comps) {
    return (comps == 1 || comps == 3) && H >= 1 && W >= 1 && H <= 65535u && W <= 65535u;
}

// ---- the codes of a BITS / HUFFVAL pair (T.81 Annex C, Figures C.1 to C.3) ----
struct HuffTabs {
    uint32_t dc[2][16];   // [luma | chroma][category]: size << 16 | code
    uint32_t ac[2][256];  // [luma | chroma][run << 4 | category]
};

constexpr void derive(const uint8_t* bits, const uint8_t* vals, uint32_t* table) {
    uint32_t code = 0, k = 0;
    for (uint32_t len = 1; len <= 16; ++len) {
        for (uint32_t i = 0; i < bits[len - 1]; ++i) table[vals[k++]] = (len << 16) | code++;
        code <<= 1;
    }
}

constexpr HuffTabs make_huff() {
    HuffTabs t{};
    derive(kJpegDcLumaBits, kJpegDcLumaVals, t.dc[0]);
    derive(kJpegDcChromaBits, kJpegDcChromaVals, t.dc[1]);
    derive(kJpegAcLumaBits, kJpegAcLumaVals, t.ac[0]);
    derive(kJpegAcChromaBits, kJpegAcChromaVals, t.ac[1]);
    return t;
}

constexpr HuffTabs kHuffHost = make_huff();
static_assert(kHuffHost.ac[0][0x00] == ((4u << 16) | 0xau), "K.5: EOB is 1010");
static_assert(kHuffHost.ac[0][0xf0] == ((11u << 16) | 0x7f9u), "K.5: ZRL is 11111111001");
static_assert(kHuffHost.ac[1][0xfa] == ((16u << 16) | 0xfffeu), "K.6: the last code");
__constant__ HuffTabs g_huff = make_huff();

// ---- launch 1: colour, DCT, quantisation, zigzag ----
struct Transform {
    float cosm[64];     // [u][x] = c(u) / 2 * cos((2 x + 1) u pi / 16), c(0) = 1 / sqrt(2): T.81 A.3.3, orthonormal
    uint16_t q[2][64];  // [luma | chroma], natural order
    uint8_t zpos[64];   // natural index -> position in the zigzag sequence
};

constexpr uint32_t kXformThreads = 256, kXformWaves = kXformThreads / kWave;

__global__ void __launch_bounds__(kXformThreads)
k_jpeg_transform(const uint8_t* __restrict__ pixels, uint32_t H, uint32_t W, uint32_t comps, uint32_t mcus_x,
                 uint32_t n_mcus, Transform t, int16_t* __restrict__ ws) {
    __shared__ float s_cos[64], s_q[2][64];
    __shared__ uint32_t s_z[64];
    __shared__ float s_a[kXformWaves][64], s_t[kXformWaves][64];
    const uint32_t wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
    if (threadIdx.x < 64) {
        s_cos[lane] = t.cosm[lane];
        s_q[0][lane] = (float)t.q[0][lane];
        s_q[1][lane] = (float)t.q[1][lane];
        s_z[lane] = t.zpos[lane];
    }
    __syncthreads();
    const uint32_t mcu_raw = blockIdx.x * kXformWaves + wave;
    const bool live = mcu_raw < n_mcus;  // (a wave past the image computes the last MCU and stores nothing)
    const uint32_t mcu = live ? mcu_raw : n_mcus - 1u;
    const uint32_t r = lane >> 3, c = lane & 7u;
    // edge blocks repeat the last column and row
    const uint32_t py = min((mcu / mcus_x) * 8u + r, H - 1u), px = min((mcu % mcus_x) * 8u + c, W - 1u);
    const size_t p = (size_t)py * W + px;
    float v[3];
    if (comps == 3) {
        const float R = (float)pixels[p * 3], G = (float)pixels[p * 3 + 1], B = (float)pixels[p * 3 + 2];
        // JFIF: Y, Cb, Cr; the + 128 of the chroma and the level shift by -128 cancel
        v[0] = ((0.299f * R + 0.587f * G) + 0.114f * B) - 128.0f;
        v[1] = (-0.168736f * R - 0.331264f * G) + 0.5f * B;
        v[2] = (0.5f * R - 0.418688f * G) - 0.081312f * B;
    } else {
        v[0] = (float)pixels[p] - 128.0f;
        v[1] = v[2] = 0.0f;
    }
    for (uint32_t comp = 0; comp < comps; ++comp) {
        s_a[wave][lane] = v[comp];
        __syncthreads();
        float acc = 0.0f;  // row pass: lane (r, u = c)
#pragma unroll
        for (uint32_t k = 0; k < 8; ++k) acc = fmaf(s_a[wave][r * 8 + k], s_cos[c * 8 + k], acc);
        s_t[wave][lane] = acc;
        __syncthreads();
        acc = 0.0f;  // column pass: lane (v = r, u = c), natural index = lane
#pragma unroll
        for (uint32_t k = 0; k < 8; ++k) acc = fmaf(s_cos[r * 8 + k], s_t[wave][k * 8 + c], acc);
        const float lim = lane == 0 ? 2047.0f : 1023.0f;
        const float f = fminf(fmaxf(rintf(acc / s_q[comp > 0][lane]), -lim), lim);
        if (live) ws[((size_t)mcu * comps + comp) * 64 + s_z[lane]] = (int16_t)f;
        // (s_a is written again only after the next barrier-separated read of s_t)
    }
}

// ---- launch 2: Huffman coding, a wave per restart interval ----
NGP_DEV int coef_at(const uint32_t* cf, uint32_t k) {
    const uint32_t w = cf[k >> 1];
    return (int)(int16_t)((k & 1u) ? (w >> 16) : (w & 0xffffu));
}

// `len` bits (the low bits of v, first bit highest) at bit `pos` of the buffer
// (word w holds stream bits 32 w .. 32 w + 31, first bit highest)
template <bool EMIT> NGP_DEV void put_bits(uint32_t* bits, uint32_t& pos, uint32_t v, uint32_t len) {
    if (EMIT && len != 0) {
        const uint32_t w = pos >> 5, off = pos & 31u;
        const uint64_t t = (uint64_t)v << (64u - off - len);  // off + len <= 31 + 27
        atomicOr(&bits[w], (uint32_t)(t >> 32));
        const uint32_t lo = (uint32_t)t;
        if (lo) atomicOr(&bits[w + 1], lo);
    }
    pos += len;
}

NGP_DEV void category(int v, uint32_t& cat, uint32_t& mag) {
    const uint32_t a = (uint32_t)(v < 0 ? -v : v);
    cat = a ? 32u - (uint32_t)__clz(a) : 0u;
    mag = (uint32_t)(v + (v >> 31)) & ((1u << cat) - 1u);  // v > 0: v; v < 0: v - 1, the low cat bits (T.81 F.1.2.1)
}

// One block (T.81 F.1.2) at bit `pos`; -> the position after it.
template <bool EMIT>
NGP_DEV uint32_t code_block(const uint32_t* cf, int pred, const uint32_t* dc, const uint32_t* ac, uint32_t* bits,
                            uint32_t pos) {
    uint32_t cat, mag;
    category(coef_at(cf, 0) - pred, cat, mag);
    uint32_t e = dc[cat & 15u];
    put_bits<EMIT>(bits, pos, ((e & 0xffffu) << cat) | mag, (e >> 16) + cat);
    uint32_t run = 0;
    for (uint32_t k = 1; k < 64; ++k) {
        const int v = coef_at(cf, k);
        if (v == 0) {
            ++run;
            continue;
        }
        for (; run >= 16; run -= 16) put_bits<EMIT>(bits, pos, ac[0xf0] & 0xffffu, ac[0xf0] >> 16);  // ZRL
        category(v, cat, mag);
        cat = min(cat, 10u);  // (the transform clamps AC to +-1023)
        mag &= (1u << cat) - 1u;
        e = ac[(run << 4) | cat];
        put_bits<EMIT>(bits, pos, ((e & 0xffffu) << cat) | mag, (e >> 16) + cat);
        run = 0;
    }
    if (run) put_bits<EMIT>(bits, pos, ac[0] & 0xffffu, ac[0] >> 16);  // EOB
    return pos;
}

NGP_DEV uint32_t stream_byte(const uint32_t* bits, uint32_t j) {
    return (bits[j >> 2] >> (24u - 8u * (j & 3u))) & 0xffu;
}

__global__ void __launch_bounds__(kWave)
k_jpeg_code(const int16_t* __restrict__ ws, uint32_t comps, uint32_t bpi, uint8_t* __restrict__ slabs,
            uint64_t slab_stride, uint32_t slab_cap, uint32_t* __restrict__ lens) {
    __shared__ uint32_t s_dc[2][16], s_ac[2][256];
    __shared__ uint32_t s_cf[kWave * kCoefStride];
    __shared__ uint32_t s_bits[kBitWords];
    const uint32_t lane = threadIdx.x, interval = blockIdx.x;
    for (uint32_t i = lane; i < 32; i += kWave) s_dc[i >> 4][i & 15u] = g_huff.dc[i >> 4][i & 15u];
    for (uint32_t i = lane; i < 512; i += kWave) s_ac[i >> 8][i & 255u] = g_huff.ac[i >> 8][i & 255u];
    for (uint32_t i = lane; i < kBitWords; i += kWave) s_bits[i] = 0u;
    const int16_t* row = ws + (size_t)interval * bpi * 64;
    const uint32_t* row32 = reinterpret_cast<const uint32_t*>(row);
    uint8_t* slab = slabs + (size_t)interval * slab_stride;
    uint32_t carry_bits = 0, carry_val = 0, out_pos = 0;  // uniform over the wave
    __syncthreads();
    for (uint32_t b0 = 0; b0 < bpi; b0 += kWave) {
        const uint32_t nb = min(kWave, bpi - b0);
        // the coefficients of nb blocks, coalesced, to a padded row per block
        for (uint32_t i = lane; i < nb * 32u; i += kWave)
            s_cf[(i >> 5) * kCoefStride + (i & 31u)] = row32[(size_t)b0 * 32u + i];
        if (lane == 0 && carry_bits) s_bits[0] = carry_val << (32u - carry_bits);
        __syncthreads();
        const uint32_t b = b0 + lane;
        const bool has = lane < nb;
        const uint32_t comp = b % comps;
        const uint32_t tab = comp > 0 ? 1u : 0u;
        // the predictor: the DC of the component's block in the MCU before, 0 at the start of the interval
        const int pred = (has && b >= comps) ? (int)row[(size_t)(b - comps) * 64] : 0;
        const uint32_t* cf = s_cf + lane * kCoefStride;
        const uint32_t len = has ? code_block<false>(cf, pred, s_dc[tab], s_ac[tab], s_bits, 0u) : 0u;
        uint32_t incl = len;
#pragma unroll
        for (uint32_t d = 1; d < kWave; d <<= 1) {
            const uint32_t up = __shfl_up(incl, d, kWave);
            if (lane >= d) incl += up;
        }
        uint32_t total = carry_bits + __shfl(incl, kWave - 1, kWave);
        if (has) code_block<true>(cf, pred, s_dc[tab], s_ac[tab], s_bits, carry_bits + incl - len);
        const bool last = b0 + kWave >= bpi;
        if (last && (total & 7u)) {  // pad the interval's last byte with ones
            const uint32_t pad = 8u - (total & 7u);
            if (lane == 0) {
                uint32_t pos = total;
                put_bits<true>(s_bits, pos, (1u << pad) - 1u, pad);
            }
            total += pad;
        }
        __syncthreads();
        const uint32_t nbytes = total >> 3;
        carry_bits = total & 7u;
        carry_val = carry_bits ? stream_byte(s_bits, nbytes) >> (8u - carry_bits) : 0u;
        // byte stuffing: 0xFF is followed by 0x00
        for (uint32_t base = 0; base < nbytes; base += kWave) {
            const uint32_t j = base + lane;
            const bool in = j < nbytes;
            const uint32_t byte = in ? stream_byte(s_bits, j) : 0u;
            const bool ff = in && byte == 0xffu;
            const uint64_t m = __ballot(ff);
            const uint32_t o = out_pos + lane + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
            if (in && o < slab_cap) slab[o] = (uint8_t)byte;
            if (ff && o + 1u < slab_cap) slab[o + 1u] = 0u;
            out_pos += min(kWave, nbytes - base) + (uint32_t)__popcll(m);
        }
        __syncthreads();
        for (uint32_t i = lane; i < (total >> 5) + 2u; i += kWave) s_bits[i] = 0u;
        __syncthreads();
    }
    if (lane == 0) lens[interval] = min(out_pos, slab_cap);
}

// ---- launch 3: the slabs and RSTm markers into one scan ----
constexpr uint32_t kCompactThreads = 256;

__global__ void __launch_bounds__(kCompactThreads)
k_jpeg_compact(const uint8_t* __restrict__ slabs, uint64_t slab_stride, const uint32_t* __restrict__ lens,
               uint32_t n_intervals, uint8_t* __restrict__ out, uint64_t capacity, uint32_t* __restrict__ out_len) {
    __shared__ uint32_t s_sum[kCompactThreads];
    const uint32_t interval = blockIdx.x;
    uint32_t acc = 0;  // the bytes before this interval: integer sums, any order gives the same
    for (uint32_t j = threadIdx.x; j < interval; j += kCompactThreads) acc += lens[j] + 2u;
    s_sum[threadIdx.x] = acc;
    __syncthreads();
    for (uint32_t o = kCompactThreads / 2; o > 0; o >>= 1) {
        if (threadIdx.x < o) s_sum[threadIdx.x] += s_sum[threadIdx.x + o];
        __syncthreads();
    }
    const uint64_t at = s_sum[0];
    const uint32_t n = lens[interval];
    const uint8_t* slab = slabs + (size_t)interval * slab_stride;
    for (uint32_t i = threadIdx.x; i < n; i += kCompactThreads)
        if (at + i < capacity) out[at + i] = slab[i];
    if (threadIdx.x == 0) {
        if (interval + 1u < n_intervals) {
            if (at + n + 1u < capacity) {
                out[at + n] = 0xffu;
                out[at + n + 1u] = (uint8_t)(0xd0u + (interval & 7u));  // RSTm, m = interval mod 8
            }
        } else {
            *out_len = (uint32_t)(at + n);
        }
    }
}

}  // namespace

extern "C" size_t ngp_jpeg_scan_capacity(uint32_t H, uint32_t W, uint32_t components) {
    return valid_shape(H, W, components) ? (size_t)layout(H, W, components).scan_cap : 0;
}

extern "C" size_t ngp_jpeg_workspace_elems(uint32_t H, uint32_t W, uint32_t components) {
    return valid_shape(H, W, components) ? (size_t)(layout(H, W, components).ws_bytes / 2) : 0;
}

extern "C" int ngp_jpeg_encode(const uint8_t* pixels, uint32_t H, uint32_t W, uint32_t components,
                               const uint16_t* qtable_luma, const uint16_t* qtable_chroma, int16_t* coef_ws,
                               uint8_t* out, size_t capacity, uint32_t* out_len, void* stream) {
    NGP_REQUIRE(components == 1 || components == 3, NGP_ERR_ARG, "jpeg_encode: components must be 1 or 3, got %u",
                components);
    NGP_REQUIRE(H >= 1 && W >= 1 && H <= 65535u && W <= 65535u, NGP_ERR_ARG,
                "jpeg_encode: H and W must be in [1, 65535], got %u x %u", H, W);
    NGP_REQUIRE(pixels && qtable_luma && (components == 1 || qtable_chroma) && coef_ws && out && out_len, NGP_ERR_ARG,
                "jpeg_encode: null buffer");
    NGP_REQUIRE((reinterpret_cast<uintptr_t>(coef_ws) & 15u) == 0 && (reinterpret_cast<uintptr_t>(out_len) & 3u) == 0,
                NGP_ERR_ARG, "jpeg_encode: coef_ws must be 16-byte aligned, out_len 4-byte aligned");
    const Layout l = layout(H, W, components);
    NGP_REQUIRE(l.scan_cap <= 0xffffffffull, NGP_ERR_ARG,
                "jpeg_encode: the worst-case scan of %u x %u x %u does not fit 32 bits", H, W, components);
    NGP_REQUIRE(capacity >= l.scan_cap, NGP_ERR_ARG,
                "jpeg_encode: capacity %zu is below ngp_jpeg_scan_capacity = %llu", capacity,
                (unsigned long long)l.scan_cap);
    Transform t;
    for (uint32_t i = 0; i < 64; ++i) {
        const uint16_t ql = qtable_luma[i], qc = components == 3 ? qtable_chroma[i] : qtable_luma[i];
        NGP_REQUIRE(ql >= 1 && ql <= 255 && qc >= 1 && qc <= 255, NGP_ERR_ARG,
                    "jpeg_encode: quantiser %u is outside 1..255 (baseline)", i);
        t.q[0][i] = ql;
        t.q[1][i] = qc;
        t.zpos[kJpegZigzag[i]] = (uint8_t)i;
    }
    const double pi = 3.14159265358979323846;
    for (uint32_t u = 0; u < 8; ++u)
        for (uint32_t x = 0; x < 8; ++x)
            t.cosm[u * 8 + x] =
                (float)((u == 0 ? std::sqrt(0.5) : 1.0) * 0.5 * std::cos((2.0 * x + 1.0) * u * pi / 16.0));
    uint8_t* base = reinterpret_cast<uint8_t*>(coef_ws);
    uint32_t* lens = reinterpret_cast<uint32_t*>(base + l.len_off);
    uint8_t* slabs = base + l.slab_off;
    hipStream_t s = ngp_stream(stream);
    k_jpeg_transform<<<ngp_div_up(l.n_mcus, kXformWaves), kXformThreads, 0, s>>>(pixels, H, W, components, l.mcus_x,
                                                                                 l.n_mcus, t, coef_ws);
    k_jpeg_code<<<l.mcus_y, kWave, 0, s>>>(coef_ws, components, l.bpi, slabs, l.slab_stride, (uint32_t)l.slab_cap,
                                           lens);
    k_jpeg_compact<<<l.mcus_y, kCompactThreads, 0, s>>>(slabs, l.slab_stride, lens, l.mcus_y, out, (uint64_t)capacity,
                                                        out_len);
    return ngp_check_launch("jpeg_encode");
}
