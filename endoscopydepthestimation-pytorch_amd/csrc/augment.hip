// Training-phase image augmentations -- reference train.py:121-142 (the albumentations pipeline) applied per frame at dataset.py:432-447,
// before Normalize(0.5, 0.5).  Arithmetic restated from albumentations 0.4.6 / OpenCV / libjpeg-turbo (tests/augment_restate.py is the
// numpy statement every kernel is checked against).
//
// A batch of F uint8 (H, W, 3) RGB frames goes through FIVE launches whatever each frame drew; the frame is blockIdx.z / .y and a per-frame
// record (endo_augment_frame, copied into the workspace) says what to do.  A frame a stage does not touch is copied through by it.
//   colour   src -> A   composed brightness-contrast + gamma LUT, then RGB -> HSV (OpenCV 8-bit, hue range 180) -> three LUTs -> RGB
//                       (OpenCV's float HSV2RGB); the LUTs and the HSV division tables live in LDS
//   spatial  A -> B     box / median / motion blur from one 22 x 22 LDS tile (16 x 16 outputs + a 3-pixel halo), border per op
//   jpeg     B -> planes (encode: one block per 16 x 16 MCU: jccolor, jcsample h2v2, jfdctint, jcdctmgr quantisation, then
//                       dequantisation + jidctint into the decoder's planes), planes -> A (decode: fancy upsampling + jdcolor)
//   noise    A -> out   GaussNoise / additive Gaussian noise from Philox4x32-10 keyed by (seed, frame, pixel), then the uint8 HWC
//                       and / or the Normalize(0.5, 0.5) fp32 CHW tensor
#include <cmath>

#include "common.h"
#include "hsv_device.h"
#include "jpeg_device.h"

namespace endo {

constexpr int kAugTile = 16;
constexpr int kAugHalo = 3;
constexpr int kAugSpan = kAugTile + 2 * kAugHalo;

__device__ __forceinline__ int aug_reflect101(int i, int n) {          // n >= 4, |overhang| <= 3
    if (i < 0) i = -i;
    if (i >= n) i = 2 * n - 2 - i;
    return i;
}

__device__ __forceinline__ int aug_replicate(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }

// ---------------------------------------------------------------------------------------------
// colour
// ---------------------------------------------------------------------------------------------
constexpr int kColourPixels = 1024;          // per block: 256 threads x 4

__global__ void __launch_bounds__(256) aug_colour_kernel(const uint8_t* __restrict__ src, const endo_augment_frame* __restrict__ prm,
                                                         uint8_t* __restrict__ dst, int64_t pixels) {
    const int f = blockIdx.y;
    const endo_augment_frame& p = prm[f];
    const uint8_t* s = src + static_cast<int64_t>(f) * pixels * 3;
    uint8_t* d = dst + static_cast<int64_t>(f) * pixels * 3;
    const int64_t base = static_cast<int64_t>(blockIdx.x) * kColourPixels;
    const int op = p.colour;
    if (op == 0) {
        for (int64_t i = base * 3 + threadIdx.x; i < min(pixels, base + kColourPixels) * 3; i += 256) d[i] = s[i];
        return;
    }
    __shared__ uint8_t lut[4][256];          // rgb, hue, sat, val
    __shared__ int sdiv[256], hdiv[256];
    const int t = threadIdx.x;
    lut[0][t] = p.rgb_lut[t];
    lut[1][t] = p.hsv_lut[0][t];
    lut[2][t] = p.hsv_lut[1][t];
    lut[3][t] = p.hsv_lut[2][t];
    sdiv[t] = t ? static_cast<int>(rint(static_cast<double>(255 << 12) / t)) : 0;          // color_hsv RGB2HSV_b tables, hrange 180
    hdiv[t] = t ? static_cast<int>(rint(static_cast<double>(180 << 12) / (6.0 * t))) : 0;
    __syncthreads();
    for (int k = 0; k < kColourPixels / 256; ++k) {
        const int64_t i = base + k * 256 + t;
        if (i >= pixels) break;
        int r = s[3 * i], g = s[3 * i + 1], b = s[3 * i + 2];
        if (op & 1) { r = lut[0][r]; g = lut[0][g]; b = lut[0][b]; }
        if (op & 2) {
            // cv2.COLOR_RGB2HSV (8 bit): v = max, s = (diff * sdiv[v] + 2048) >> 12, h = (hterm * hdiv[diff] + 2048) >> 12, + 180 if < 0
            const int v = max(max(b, g), r), vmin = min(min(b, g), r), diff = v - vmin;
            const int sat = (diff * sdiv[v] + (1 << 11)) >> 12;
            const int hterm = v == r ? g - b : (v == g ? b - r + 2 * diff : r - g + 4 * diff);
            int h = (hterm * hdiv[diff] + (1 << 11)) >> 12;
            h += h < 0 ? 180 : 0;
            h = h > 255 ? 255 : h;
            int rgb[3];
            hsv_to_rgb<180>(lut[1][h], lut[2][sat], lut[3][v], rgb);          // cv2.COLOR_HSV2RGB
            r = rgb[0]; g = rgb[1]; b = rgb[2];
        }
        d[3 * i] = static_cast<uint8_t>(r);
        d[3 * i + 1] = static_cast<uint8_t>(g);
        d[3 * i + 2] = static_cast<uint8_t>(b);
    }
}

// ---------------------------------------------------------------------------------------------
// spatial
// ---------------------------------------------------------------------------------------------
// median of K*K bytes: radix selection, MSB first -- the largest m with #(x < m) <= (K*K - 1) / 2
template <int K>
__device__ __forceinline__ int median_at(const uint8_t (*tile)[kAugSpan], int ty, int tx) {
    constexpr int R = K / 2, N = K * K, MID = (N - 1) / 2;
    int v[N];
#pragma unroll
    for (int i = 0; i < K; ++i)
#pragma unroll
        for (int j = 0; j < K; ++j) v[i * K + j] = tile[ty + kAugHalo - R + i][tx + kAugHalo - R + j];
    int m = 0;
#pragma unroll
    for (int bit = 7; bit >= 0; --bit) {
        const int cand = m | (1 << bit);
        int below = 0;
#pragma unroll
        for (int i = 0; i < N; ++i) below += v[i] < cand;
        m = below <= MID ? cand : m;
    }
    return m;
}

__global__ void __launch_bounds__(256) aug_spatial_kernel(const uint8_t* __restrict__ src, const endo_augment_frame* __restrict__ prm,
                                                          uint8_t* __restrict__ dst, int height, int width) {
    const int f = blockIdx.z;
    const endo_augment_frame& p = prm[f];
    const int64_t frame_off = static_cast<int64_t>(f) * height * width * 3;
    const uint8_t* s = src + frame_off;
    uint8_t* d = dst + frame_off;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int y0 = blockIdx.y * kAugTile, x0 = blockIdx.x * kAugTile;
    const int x = x0 + tx, y = y0 + ty;
    const int op = p.spatial;
    if (op == 0) {
        if (x < width && y < height) {
            const int64_t o = (static_cast<int64_t>(y) * width + x) * 3;
            d[o] = s[o]; d[o + 1] = s[o + 1]; d[o + 2] = s[o + 2];
        }
        return;
    }
    __shared__ uint8_t tile[3][kAugSpan][kAugSpan];
    for (int i = threadIdx.x; i < kAugSpan * kAugSpan; i += 256) {
        const int ly = i / kAugSpan, lx = i - ly * kAugSpan;
        const int gy = y0 + ly - kAugHalo, gx = x0 + lx - kAugHalo;
        // cv2.medianBlur: BORDER_REPLICATE; cv2.blur / cv2.filter2D: BORDER_REFLECT_101.  Far-off tile cells are never read, but clamped.
        const int sy = op == 2 ? aug_replicate(gy, height) : aug_replicate(aug_reflect101(gy, height), height);
        const int sx = op == 2 ? aug_replicate(gx, width) : aug_replicate(aug_reflect101(gx, width), width);
        const int64_t o = (static_cast<int64_t>(sy) * width + sx) * 3;
        tile[0][ly][lx] = s[o];
        tile[1][ly][lx] = s[o + 1];
        tile[2][ly][lx] = s[o + 2];
    }
    __syncthreads();
    if (x >= width || y >= height) return;
    const int k = p.ksize, r = k / 2;
    int out[3];
    if (op == 1) {          // cv2.blur: sum / k^2 rounded to nearest (k^2 odd: no ties)
        for (int c = 0; c < 3; ++c) {
            int sum = 0;
            for (int i = -r; i <= r; ++i)
                for (int j = -r; j <= r; ++j) sum += tile[c][ty + kAugHalo + i][tx + kAugHalo + j];
            out[c] = (2 * sum + k * k) / (2 * k * k);
        }
    } else if (op == 2) {
        for (int c = 0; c < 3; ++c)
            out[c] = k == 3 ? median_at<3>(tile[c], ty, tx) : (k == 5 ? median_at<5>(tile[c], ty, tx) : median_at<7>(tile[c], ty, tx));
    } else {                // motion blur: mean of the n marked taps (correlation, centre anchor), rounded half to even
        const uint64_t mask = static_cast<uint64_t>(p.motion[0]) | (static_cast<uint64_t>(p.motion[1]) << 32);
        const int n = __popcll(mask);
        for (int c = 0; c < 3; ++c) {
            int sum = 0;
            for (int i = 0; i < k; ++i)
                for (int j = 0; j < k; ++j)
                    if ((mask >> (i * k + j)) & 1) sum += tile[c][ty + kAugHalo - r + i][tx + kAugHalo - r + j];
            int q = sum / n;
            const int rem2 = 2 * (sum - q * n);
            q += rem2 > n || (rem2 == n && (q & 1));
            out[c] = q;
        }
    }
    const int64_t o = (static_cast<int64_t>(y) * width + x) * 3;
    d[o] = static_cast<uint8_t>(out[0]); d[o + 1] = static_cast<uint8_t>(out[1]); d[o + 2] = static_cast<uint8_t>(out[2]);
}

// ---------------------------------------------------------------------------------------------
// JPEG round trip
// ---------------------------------------------------------------------------------------------
struct AugJpegGeom {
    int mcus_x, mcus_y, ystride, cstride, cw, ch;
    int64_t frame_bytes, cb_off, cr_off;
};

static AugJpegGeom aug_jpeg_geom(int height, int width) {
    AugJpegGeom g;
    g.mcus_x = (width + 15) / 16;
    g.mcus_y = (height + 15) / 16;
    g.ystride = g.mcus_x * 16;
    g.cstride = g.mcus_x * 8;
    g.cw = (width + 1) / 2;
    g.ch = (height + 1) / 2;
    const int64_t ybytes = static_cast<int64_t>(g.ystride) * g.mcus_y * 16, cbytes = static_cast<int64_t>(g.cstride) * g.mcus_y * 8;
    g.cb_off = ybytes;
    g.cr_off = ybytes + cbytes;
    g.frame_bytes = (ybytes + 2 * cbytes + 255) & ~static_cast<int64_t>(255);
    return g;
}

// jfdctint.c (jpeg_fdct_islow), one pass over 8 samples; pass 1 (rows) keeps PASS1_BITS of extra precision, pass 2 (columns) removes it
__device__ __forceinline__ void fdct_islow_1d(int (&d)[8], bool first) {
    const int tmp0 = d[0] + d[7], tmp7 = d[0] - d[7], tmp1 = d[1] + d[6], tmp6 = d[1] - d[6];
    const int tmp2 = d[2] + d[5], tmp5 = d[2] - d[5], tmp3 = d[3] + d[4], tmp4 = d[3] - d[4];
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    const int shift = first ? 13 - 2 : 13 + 2;
    const int rnd = 1 << (shift - 1);
    if (first) {
        d[0] = (tmp10 + tmp11) * 4;
        d[4] = (tmp10 - tmp11) * 4;
    } else {
        d[0] = (tmp10 + tmp11 + 2) >> 2;
        d[4] = (tmp10 - tmp11 + 2) >> 2;
    }
    int z1 = (tmp12 + tmp13) * 4433;
    d[2] = (z1 + tmp13 * 6270 + rnd) >> shift;
    d[6] = (z1 + tmp12 * (-15137) + rnd) >> shift;
    z1 = tmp4 + tmp7;
    int z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
    const int z5 = (z3 + z4) * 9633;
    const int t4 = tmp4 * 2446, t5 = tmp5 * 16819, t6 = tmp6 * 25172, t7 = tmp7 * 12299;
    z1 *= -7373; z2 *= -20995; z3 *= -16069; z4 *= -3196;
    z3 += z5; z4 += z5;
    d[7] = (t4 + z1 + z3 + rnd) >> shift;
    d[5] = (t5 + z2 + z4 + rnd) >> shift;
    d[3] = (t6 + z2 + z3 + rnd) >> shift;
    d[1] = (t7 + z1 + z4 + rnd) >> shift;
}

// jcdctmgr.c (libjpeg-turbo) quantize(): divisor = 8 q, reciprocal / correction / shift of compute_reciprocal()
__device__ __forceinline__ int quantize(int temp, int q) {
    const unsigned divisor = 8u * static_cast<unsigned>(q);
    const int b = 31 - __clz(divisor);
    int r = 16 + b;
    unsigned fq = (1u << r) / divisor;
    const unsigned fr = (1u << r) % divisor;
    unsigned c = divisor / 2;
    if (fr == 0) { fq >>= 1; --r; }
    else if (fr <= divisor / 2) ++c;
    else ++fq;
    const unsigned a = static_cast<unsigned>(temp < 0 ? -temp : temp);
    const int v = static_cast<int>(((a + c) * fq) >> r);
    return temp < 0 ? -v : v;
}

// one 16 x 16 MCU (4 Y blocks, Cb, Cr) per 64-thread block
__global__ void __launch_bounds__(64) aug_jpeg_encode_kernel(const uint8_t* __restrict__ src, const endo_augment_frame* __restrict__ prm,
                                                             uint8_t* __restrict__ planes, int height, int width, const AugJpegGeom g) {
    const int f = blockIdx.z;
    const endo_augment_frame& p = prm[f];
    if (!p.jpeg) return;
    const uint8_t* s = src + static_cast<int64_t>(f) * height * width * 3;
    uint8_t* pl = planes + static_cast<int64_t>(f) * g.frame_bytes;
    const int mx = blockIdx.x, my = blockIdx.y, t = threadIdx.x;
    __shared__ int cbf[16][16], crf[16][16];
    __shared__ int blk[6][64];          // Y00 Y01 Y10 Y11 Cb Cr, natural order
    // jccolor.c rgb_ycc_convert (SCALEBITS 16) on the image extended to whole MCUs by edge replication (jcsample expand_right_edge,
    // jcprepct expand_bottom_edge).  cv2.imencode reads the RGB array as B, G, R: libjpeg's R is channel 2, its B channel 0.
    for (int i = t; i < 256; i += 64) {
        const int ly = i >> 4, lx = i & 15;
        const int gy = min(my * 16 + ly, height - 1), gx = min(mx * 16 + lx, width - 1);
        const uint8_t* px = s + (static_cast<int64_t>(gy) * width + gx) * 3;
        const int R = px[2], G = px[1], B = px[0];
        const int y = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16;
        cbf[ly][lx] = (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16;
        crf[ly][lx] = (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16;
        blk[(ly >> 3) * 2 + (lx >> 3)][(ly & 7) * 8 + (lx & 7)] = y - 128;
    }
    __syncthreads();
    {   // jcsample.c h2v2_downsample: (a + b + c + d + bias) >> 2 with bias 1, 2, 1, 2 along a row; chroma rows past ceil(H / 2) repeat
        // the last real one (jcprepct pads the downsampled rows to the MCU height)
        const int cy = t >> 3, cx = t & 7;
        const int ry = min(my * 8 + cy, g.ch - 1) - my * 8;
        const int bias = (cx & 1) ? 2 : 1;
        blk[4][t] = ((cbf[2 * ry][2 * cx] + cbf[2 * ry][2 * cx + 1] + cbf[2 * ry + 1][2 * cx] + cbf[2 * ry + 1][2 * cx + 1] + bias) >> 2) - 128;
        blk[5][t] = ((crf[2 * ry][2 * cx] + crf[2 * ry][2 * cx + 1] + crf[2 * ry + 1][2 * cx] + crf[2 * ry + 1][2 * cx + 1] + bias) >> 2) - 128;
    }
    __syncthreads();
    const int b = t >> 3, line = t & 7;          // 48 of the 64 threads: one row / column of one of the six blocks
    if (b < 6) {          // FDCT pass 1: rows
        int v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = blk[b][line * 8 + k];
        fdct_islow_1d(v, true);
#pragma unroll
        for (int k = 0; k < 8; ++k) blk[b][line * 8 + k] = v[k];
    }
    __syncthreads();
    if (b < 6) {          // pass 2: columns, then quantise and dequantise the column (jcdctmgr / jddctmgr)
        const uint16_t* q = p.quant[b < 4 ? 0 : 1];
        int v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = blk[b][k * 8 + line];
        fdct_islow_1d(v, false);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int qq = q[k * 8 + line];
            v[k] = quantize(v[k], qq) * qq;
        }
        int o[8];          // jidctint pass 1 over the same column
        idct_islow_1d(v, o, 13 - 2);
#pragma unroll
        for (int k = 0; k < 8; ++k) blk[b][k * 8 + line] = o[k];
    }
    __syncthreads();
    if (b < 6) {          // jidctint pass 2: rows, range limit, into the decoder's planes
        int v[8], o[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = blk[b][line * 8 + k];
        idct_islow_1d(v, o, 13 + 2 + 3);
        uint8_t* row;
        if (b < 4) row = pl + static_cast<int64_t>(my * 16 + (b >> 1) * 8 + line) * g.ystride + mx * 16 + (b & 1) * 8;
        else row = pl + (b == 4 ? g.cb_off : g.cr_off) + static_cast<int64_t>(my * 8 + line) * g.cstride + mx * 8;
#pragma unroll
        for (int k = 0; k < 8; ++k) row[k] = idct_range_limit(o[k]);
    }
}

// one thread per pixel: libjpeg's fancy h2v2 upsampling + YCbCr -> RGB, written back in the array's order (cv2.imdecode gives B, G, R)
__global__ void __launch_bounds__(256) aug_jpeg_decode_kernel(const uint8_t* __restrict__ src, const endo_augment_frame* __restrict__ prm,
                                                              const uint8_t* __restrict__ planes, uint8_t* __restrict__ dst, int height,
                                                              int width, const AugJpegGeom g) {
    const int f = blockIdx.y;
    const int64_t pixels = static_cast<int64_t>(height) * width;
    const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= pixels) return;
    const int64_t o = static_cast<int64_t>(f) * pixels * 3 + 3 * i;
    if (!prm[f].jpeg) {
        dst[o] = src[o]; dst[o + 1] = src[o + 1]; dst[o + 2] = src[o + 2];
        return;
    }
    const int y = static_cast<int>(i / width), x = static_cast<int>(i - static_cast<int64_t>(y) * width);
    const uint8_t* pl = planes + static_cast<int64_t>(f) * g.frame_bytes;
    const int lum = pl[static_cast<int64_t>(y) * g.ystride + x];
    const int cb = chroma_at(pl + g.cb_off, g.cstride, g.cw, g.ch, 2, 2, y, x);
    const int cr = chroma_at(pl + g.cr_off, g.cstride, g.cw, g.ch, 2, 2, y, x);
    int rgb[3];
    ycc_to_rgb(lum, cb, cr, rgb);
    dst[o] = static_cast<uint8_t>(rgb[2]);
    dst[o + 1] = static_cast<uint8_t>(rgb[1]);
    dst[o + 2] = static_cast<uint8_t>(rgb[0]);
}

// ---------------------------------------------------------------------------------------------
// noise + Normalize
// ---------------------------------------------------------------------------------------------
// Philox4x32-10 (Salmon et al., SC'11): counter (pixel, frame, 0, 0), key = the frame's 64-bit seed
__device__ __forceinline__ uint4 philox4x32_10(uint4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const uint32_t lo0 = 0xD2511F53u * c.x, hi0 = __umulhi(0xD2511F53u, c.x);
        const uint32_t lo1 = 0xCD9E8D57u * c.z, hi1 = __umulhi(0xCD9E8D57u, c.z);
        c = make_uint4(hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0);
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c;
}

// Box-Muller on two 24-bit uniforms in (0, 1)
__device__ __forceinline__ void box_muller(uint32_t a, uint32_t b, float& n0, float& n1) {
    const float u1 = (static_cast<float>(a >> 8) + 0.5f) * (1.0f / 16777216.0f);
    const float u2 = (static_cast<float>(b >> 8) + 0.5f) * (1.0f / 16777216.0f);
    const float rad = sqrtf(-2.0f * logf(u1));
    float sn, cs;
    sincospif(2.0f * u2, &sn, &cs);
    n0 = rad * cs;
    n1 = rad * sn;
}

__global__ void __launch_bounds__(256) aug_noise_kernel(const uint8_t* __restrict__ src, const endo_augment_frame* __restrict__ prm,
                                                        int64_t pixels, uint8_t* __restrict__ out_u8, float* __restrict__ out_f32) {
    const int f = blockIdx.y;
    const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= pixels) return;
    const endo_augment_frame& p = prm[f];
    const int64_t o = static_cast<int64_t>(f) * pixels * 3 + 3 * i;
    int v[3] = {src[o], src[o + 1], src[o + 2]};
    if (p.noise) {
        const uint4 bits = philox4x32_10(make_uint4(static_cast<uint32_t>(i), static_cast<uint32_t>(f), 0u, 0u), p.seed[0], p.seed[1]);
        float n[4];
        box_muller(bits.x, bits.y, n[0], n[1]);
        box_muller(bits.z, bits.w, n[2], n[3]);
        for (int c = 0; c < 3; ++c) {
            if (p.noise == 1) {          // GaussNoise: clip(float(v) + sigma * n_c, 0, 255), truncated
                const float a = fminf(fmaxf(static_cast<float>(v[c]) + p.sigma * n[c], 0.0f), 255.0f);
                v[c] = static_cast<int>(a);
            } else {                     // imgaug AdditiveGaussianNoise(per_channel=False): one draw per pixel, rounded half to even
                v[c] = clamp255(static_cast<int>(rintf(static_cast<float>(v[c]) + p.sigma * n[0])));
            }
        }
    }
    if (out_u8) { out_u8[o] = static_cast<uint8_t>(v[0]); out_u8[o + 1] = static_cast<uint8_t>(v[1]); out_u8[o + 2] = static_cast<uint8_t>(v[2]); }
    if (out_f32) {          // albumentations Normalize(mean 0.5, std 0.5, max_pixel_value 255) in fp32, CHW
        float* d = out_f32 + static_cast<int64_t>(f) * pixels * 3 + i;
        for (int c = 0; c < 3; ++c) d[c * pixels] = (static_cast<float>(v[c]) - 127.5f) * (1.0f / 127.5f);
    }
}

struct AugLayout {
    int64_t params, a, b, planes, total;
};

static AugLayout aug_layout(int frames, int height, int width) {
    AugLayout l;
    const int64_t img = static_cast<int64_t>(frames) * height * width * 3;
    l.params = 0;
    l.a = align256(static_cast<int64_t>(frames) * sizeof(endo_augment_frame));
    l.b = l.a + align256(img);
    l.planes = l.b + align256(img);
    l.total = l.planes + frames * aug_jpeg_geom(height, width).frame_bytes;
    return l;
}

static bool aug_frame_ok(const endo_augment_frame& p) {
    if (p.colour < 0 || p.colour > 3 || p.spatial < 0 || p.spatial > 3 || (p.jpeg != 0 && p.jpeg != 1) || p.noise < 0 || p.noise > 2) return false;
    if (p.spatial) {
        if (p.ksize != 3 && p.ksize != 5 && p.ksize != 7) return false;
        if (p.spatial == 3) {
            const uint64_t mask = static_cast<uint64_t>(p.motion[0]) | (static_cast<uint64_t>(p.motion[1]) << 32);
            const int kk = p.ksize * p.ksize;
            if (mask == 0 || (kk < 64 && (mask >> kk) != 0)) return false;
        }
    }
    if (p.jpeg)
        for (int t = 0; t < 2; ++t)
            for (int i = 0; i < 64; ++i)
                if (p.quant[t][i] < 1 || p.quant[t][i] > 255) return false;
    if (p.noise && !(p.sigma >= 0.0f && p.sigma < 1.0e4f)) return false;
    return true;
}

}  // namespace endo

using namespace endo;

extern "C" int endo_augment_frame_bytes(void) { return static_cast<int>(sizeof(endo_augment_frame)); }

extern "C" int64_t endo_augment_workspace_bytes(int frames, int height, int width) {
    if (frames <= 0 || height < 4 || width < 4) return -1;
    return aug_layout(frames, height, width).total;
}

extern "C" int endo_augment(const uint8_t* src, const endo_augment_frame* params, int frames, int height, int width, uint8_t* out_u8,
                            float* out_f32, void* workspace, int64_t workspace_bytes, void* stream_) {
    if (!src || !params || !workspace || (!out_u8 && !out_f32)) return ENDO_E_BADARG;
    if (frames <= 0 || frames > 65535 || height < 4 || width < 4 || static_cast<int64_t>(height) * width > (int64_t(1) << 30)) return ENDO_E_BADARG;
    for (int f = 0; f < frames; ++f)
        if (!aug_frame_ok(params[f])) return ENDO_E_UNSUPPORTED;
    const AugLayout l = aug_layout(frames, height, width);
    if (workspace_bytes < l.total) return ENDO_E_BADARG;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    char* ws = static_cast<char*>(workspace);
    const endo_augment_frame* prm = reinterpret_cast<const endo_augment_frame*>(ws + l.params);
    uint8_t* a = reinterpret_cast<uint8_t*>(ws + l.a);
    uint8_t* b = reinterpret_cast<uint8_t*>(ws + l.b);
    uint8_t* planes = reinterpret_cast<uint8_t*>(ws + l.planes);
    ENDO_CHECK(hipMemcpyAsync(ws + l.params, params, static_cast<size_t>(frames) * sizeof(endo_augment_frame), hipMemcpyHostToDevice, stream));
    const int64_t pixels = static_cast<int64_t>(height) * width;
    const AugJpegGeom g = aug_jpeg_geom(height, width);
    ProfScope prof(kProfSmall, stream, 0.0, 0.0);
    aug_colour_kernel<<<dim3(static_cast<unsigned>((pixels + kColourPixels - 1) / kColourPixels), frames), 256, 0, stream>>>(src, prm, a, pixels);
    aug_spatial_kernel<<<dim3((width + kAugTile - 1) / kAugTile, (height + kAugTile - 1) / kAugTile, frames), 256, 0, stream>>>(a, prm, b, height, width);
    aug_jpeg_encode_kernel<<<dim3(g.mcus_x, g.mcus_y, frames), 64, 0, stream>>>(b, prm, planes, height, width, g);
    aug_jpeg_decode_kernel<<<dim3(static_cast<unsigned>((pixels + 255) / 256), frames), 256, 0, stream>>>(b, prm, planes, a, height, width, g);
    aug_noise_kernel<<<dim3(static_cast<unsigned>((pixels + 255) / 256), frames), 256, 0, stream>>>(a, prm, pixels, out_u8, out_f32);
    ENDO_LAUNCH_CHECK();
    return 0;
}
