// Joint bilateral upsampling of a downscaled run's disparity map (dsx_upsample of dsx.h; host restatement
// depthestimation_amd/upsample.py, equal bit for bit): one stateless launch reads the finished low-resolution
// map d (h x w, column 0 = low-resolution column x0), the low-resolution guide g the matcher ran on (h x Wl,
// uncropped) and the full-size frame G (H x W x ch) and writes the full-size disparity, in full-size pixels,
// and the metric depth.  Per output pixel P = (X, Y), with r the radius:
//
//   near(X) = ((2X + 1) O) div (2 I);  taps k = near + t - r, t = 0..2r;  n = |(2X + 1) O - (2k + 1) I|
//   tent a(X, t) = max(0, 64 - ((64 n + (r + 1) I) div (2 (r + 1) I)))
//   W_q = a_x a_y T[|G(P) - g(q)|] over the valid (0 < d < inf) taps inside the map;  S = sum of the W_q
//   m = the smallest valid tap value v with 2 sum(W_q : d_q <= v) >= S                    (the selection)
//   a = (sum of (float)W_q d_q over |d_q - m| <= max_diff, in window order) / (float)(sum of those W_q)
//   out = a * sx;  depth = the depth map's rule on a;  no valid tap: out = the bits of the centre tap
//
// every float operation correctly rounded and uncontracted.
//
// A block of 256 threads owns kTW x kTH = 256 x 8 output pixels; a lane owns 4 consecutive pixels of a row (a
// wave writes one 256-pixel row segment: 1 KiB per store instruction on the 16-byte path) and two rows, 4 apart.
//   upsample_joint<R, VEC>
//     geometry  thread t computes near and the 2R + 1 tents of tile column t, threads 0..7 those of the tile's
//               rows, into LDS: 32-bit integers only.  With p = (2X + 1) O < 2^31, near = p div 2I and
//               c = p - near 2I - I in [-I, I), the tap's n is |c - 2 (t - R) I| <= (2R + 1) I, so 64 n +
//               (R + 1) I < 2^24: no tent is ever 0, and every valid tap weighs at least 1.
//     staging   near is monotone with steps of at most 1 (O <= I), so the tile's low-resolution footprint is
//               at most (kTH + 2R) x (kTW + 2R): it goes to LDS as 8-byte {bits of d, guide} records (one read
//               per tap), taps outside the map as +0 (invalid).  Only the rows and columns the tile needs are
//               loaded.
//     taps      a pixel's (2R + 1)^2 values and weights live in registers (loops unrolled, static indices: no
//               scratch).  The selection counts ranks directly: for every tap the weights of the taps not above
//               it are summed - from the registers at R = 1; at R > 1 the tap is re-read from LDS in a rolled
//               row loop, to keep the code small.
//     VEC       output rows are 16-byte aligned: float4 stores of disparity and depth; otherwise scalar stores.
// No atomics, no block waits on another, no workspace.
#include "dsx_internal.h"

#include <cmath>
#include <string>

#include "../../include/dsx.h"

namespace dsx {
int set_error(int code, const std::string &msg);  // dsx_api.hip: the message behind dsx_last_error
}

namespace {

constexpr int kTW = DSX_UPSAMPLE_TILE_W, kTH = DSX_UPSAMPLE_TILE_H, kThreads = 256;
constexpr int kRowsPerThread = kTH / (kThreads / 64);
constexpr int kMaxDim = 32768;
static_assert(kTW == 64 * 4, "a wave covers one row segment of the tile, 4 pixels per lane");
static_assert(kTW == kThreads, "thread t computes the geometry of tile column t");
static_assert(kTH % (kThreads / 64) == 0, "every wave owns whole rows");

struct UpTable {
    uint16_t t[256];
};

struct UpArgs {
    const uint32_t *d;  // the map's bits
    int64_t dpitch;     // elements
    const uint8_t *g;
    int64_t gstride;  // bytes
    const uint8_t *G;
    int64_t Gstride;  // bytes
    float *out, *depth;  // contiguous H x Wo (depth may be null)
    int h, w, x0, Wl;
    int H, W, ch;
    int X0, Wo;  // first output column, W - X0
    float max_diff, sx;
    float fB, doffs, eps, max_depth;
    int has_max;
};

__device__ __forceinline__ uint32_t load_u32(const uint8_t *p) {  // any alignment
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}

// near and c = (2X + 1) O - (2 near + 1) I of hi-res index X: 32-bit integers (X < I <= 32768, O <= I)
__device__ __forceinline__ int up_near(int X, int I, int O, int &c) {
    const uint32_t p = (uint32_t)(2 * X + 1) * (uint32_t)O;
    const uint32_t q = p / (uint32_t)(2 * I);
    c = (int)(p - q * (uint32_t)(2 * I)) - I;
    return (int)q;
}

template <int R>
__device__ __forceinline__ uint32_t up_tent(int c, int t, int I) {
    const uint32_t n = (uint32_t)abs(c - 2 * (t - R) * I);
    const uint32_t q = (64u * n + (uint32_t)((R + 1) * I)) / (uint32_t)(2 * (R + 1) * I);
    return q >= 64u ? 0u : 64u - q;
}

__device__ __forceinline__ bool up_valid(float v) { return v > 0.0f && v < __builtin_inff(); }

#pragma clang fp contract(off)

__device__ __forceinline__ float up_depth(const UpArgs &a, float v) {
    const float adj = v + a.doffs;
    float z = adj > a.eps ? __fdiv_rn(a.fB, adj) : __builtin_inff();
    if (a.has_max && z > a.max_depth) z = a.max_depth;
    return z;
}

// One output pixel.  rec: the staged footprint at the pixel's window origin (pitch FP); ax / ay: the tents;
// gp: G(P).  Returns the disparity in full-size pixels and, in z, the depth.
template <int R, int FP>
__device__ __forceinline__ float up_pixel(const UpArgs &a, const uint2 *rec, const uint32_t *wt,
                                          const uint32_t (&ax)[2 * R + 1], const uint32_t (&ay)[2 * R + 1], int gp,
                                          float &z) {
    constexpr int N = 2 * R + 1;
    float dv[N * N];
    uint32_t wv[N * N];
    uint32_t S = 0;
#pragma unroll
    for (int j = 0; j < N; ++j) {
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const uint2 e = rec[j * FP + i];
            const float v = __uint_as_float(e.x);
            const bool ok = up_valid(v);
            const uint32_t wq = ax[i] * ay[j] * wt[abs(gp - (int)e.y)];
            dv[j * N + i] = ok ? v : __builtin_inff();
            wv[j * N + i] = ok ? wq : 0u;
            S += wv[j * N + i];
        }
    }
    if (S == 0) {  // no valid tap: the centre tap's bits, unscaled
        const float v = __uint_as_float(rec[R * FP + R].x);
        z = up_depth(a, v);
        return v;
    }
    // the selection: the smallest valid value whose rank sum reaches half of S
    float m = __builtin_inff();
    if constexpr (R == 1) {
#pragma unroll
        for (int q = 0; q < N * N; ++q) {
            const float v = dv[q];  // +inf for an invalid tap
            uint32_t cum = 0;
#pragma unroll
            for (int p = 0; p < N * N; ++p) cum += dv[p] <= v ? wv[p] : 0u;
            if (v < __builtin_inff() && 2u * cum >= S) m = fminf(m, v);
        }
    } else {
#pragma unroll 1
        for (int j = 0; j < N; ++j) {
#pragma unroll
            for (int i = 0; i < N; ++i) {
                const float v = __uint_as_float(rec[j * FP + i].x);
                uint32_t cum = 0;
#pragma unroll
                for (int p = 0; p < N * N; ++p) cum += dv[p] <= v ? wv[p] : 0u;
                if (up_valid(v) && 2u * cum >= S) m = fminf(m, v);
            }
        }
    }
    // the gated average around it, in window order
    float num = 0.0f;
    uint32_t den = 0;
#pragma unroll
    for (int p = 0; p < N * N; ++p) {
        const float diff = dv[p] - m;
        const bool in = __builtin_fabsf(diff) <= a.max_diff;  // an invalid tap: inf - m = inf
        const float prod = (float)wv[p] * (in ? dv[p] : 0.0f);
        num = in ? num + prod : num;
        den += in ? wv[p] : 0u;
    }
    const float avg = __fdiv_rn(num, (float)den);
    z = up_depth(a, avg);
    return avg * a.sx;
}

#pragma clang fp contract(on)

template <int R, bool VEC>
__global__ __launch_bounds__(kThreads) void upsample_joint(UpArgs a, UpTable tab) {
    static_assert(R >= 1 && R <= 3, "radius 1..3");
    constexpr int N = 2 * R + 1;
    constexpr int FP = kTW + 2 * R, FH = kTH + 2 * R;  // the footprint's pitch and rows
    __shared__ uint2 rec[FH * FP];  // {bits of d, guide}
    __shared__ uint32_t wt[256];
    __shared__ __attribute__((aligned(8))) uint16_t cnear[kTW];  // near_x - near_x of the tile's first column
    __shared__ __attribute__((aligned(4))) uint8_t cten[N][kTW];
    __shared__ int rnear[kTH];  // near_y - near_y of the tile's first row
    __shared__ uint32_t rten[N][kTH];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int xo0 = blockIdx.x * kTW, y0 = blockIdx.y * kTH;  // output coordinates of the tile
    int c;
    // uniform: the footprint's origin and extent
    const int nxf = up_near(a.X0 + xo0, a.W, a.Wl, c);
    const int nxl = up_near(min(a.X0 + xo0 + kTW - 1, a.W - 1), a.W, a.Wl, c);
    const int nyf = up_near(y0, a.H, a.h, c);
    const int nyl = up_near(min(y0 + kTH - 1, a.H - 1), a.H, a.h, c);
    const int ncols = nxl - nxf + N, nrows = nyl - nyf + N;  // <= FP, <= FH
    wt[tid] = tab.t[tid];
    {
        const int X = min(a.X0 + xo0 + tid, a.W - 1);
        cnear[tid] = (uint16_t)(up_near(X, a.W, a.Wl, c) - nxf);
#pragma unroll
        for (int t = 0; t < N; ++t) cten[t][tid] = (uint8_t)up_tent<R>(c, t, a.W);
    }
    if (tid < kTH) {
        const int Y = min(y0 + tid, a.H - 1);
        rnear[tid] = up_near(Y, a.H, a.h, c) - nyf;
#pragma unroll
        for (int t = 0; t < N; ++t) rten[t][tid] = up_tent<R>(c, t, a.H);
    }
    for (int ty = wave; ty < nrows; ty += kThreads / 64) {
        const int y = nyf - R + ty;
        const bool yin = y >= 0 && y < a.h;
        const uint32_t *drow = a.d + (int64_t)(yin ? y : 0) * a.dpitch;
        const uint8_t *grow = a.g + (int64_t)(yin ? y : 0) * a.gstride;
        for (int tx = lane; tx < ncols; tx += 64) {
            const int x = nxf - R + tx;
            const bool in = yin && x >= a.x0 && x - a.x0 < a.w;
            rec[ty * FP + tx] = in ? make_uint2(drow[x - a.x0], grow[x]) : make_uint2(0u, 0u);
        }
    }
    __syncthreads();
    const int xo = xo0 + 4 * lane;
    if (xo >= a.Wo) return;
    const bool whole = xo + 3 < a.Wo;  // VEC: always (Wo is a multiple of 4)
    const uint2 nl = *reinterpret_cast<const uint2 *>(cnear + 4 * lane);
    uint32_t tw[N];
#pragma unroll
    for (int t = 0; t < N; ++t) tw[t] = *reinterpret_cast<const uint32_t *>(&cten[t][4 * lane]);
#pragma unroll 1
    for (int it = 0; it < kRowsPerThread; ++it) {
        const int ty = wave + it * (kThreads / 64), Y = y0 + ty;
        if (Y >= a.H) break;
        // G(P) of the lane's pixels
        const uint8_t *Gp = a.G + (int64_t)Y * a.Gstride + (int64_t)(a.X0 + xo) * a.ch;
        uint32_t gq = 0;  // 4 gray bytes
        if (a.ch == 1) {
            if (whole) {
                gq = load_u32(Gp);
            } else {
                for (int k = 0; k < a.Wo - xo; ++k) gq |= (uint32_t)Gp[k] << (8 * k);
            }
        } else {
            uint32_t b[3] = {0u, 0u, 0u};  // 12 bytes: 4 pixels x 3 channels in memory order
            if (whole) {
                b[0] = load_u32(Gp), b[1] = load_u32(Gp + 4), b[2] = load_u32(Gp + 8);
            } else {
                for (int k = 0; k < 3 * (a.Wo - xo); ++k) {
                    const uint32_t v = (uint32_t)Gp[k] << (8 * (k & 3));
                    b[0] |= k < 4 ? v : 0u;
                    b[1] |= k >= 4 && k < 8 ? v : 0u;
                    b[2] |= k >= 8 ? v : 0u;
                }
            }
            const uint64_t lo = ((uint64_t)b[1] << 32) | b[0];
            const uint64_t hi = ((uint64_t)b[2] << 32) | b[1];  // bytes 4..11
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t px = k < 2 ? (uint32_t)(lo >> (24 * k)) : (uint32_t)(hi >> (24 * k - 32));
                const uint32_t c0 = px & 0xFFu, c1 = (px >> 8) & 0xFFu, c2 = (px >> 16) & 0xFFu;
                gq |= ((c0 * 1868u + c1 * 9617u + c2 * 4899u + 8192u) >> 14) << (8 * k);
            }
        }
        const int lrow = rnear[ty];
        uint32_t ay[N];
#pragma unroll
        for (int t = 0; t < N; ++t) ay[t] = rten[t][ty];
        float ox = 0.0f, oy = 0.0f, oz = 0.0f, ow = 0.0f, zx = 0.0f, zy = 0.0f, zz = 0.0f, zw = 0.0f;
#pragma unroll 1
        for (int k = 0; k < 4; ++k) {
            if (xo + k >= a.Wo) break;
            const int lcol = (int)(((k < 2 ? nl.x : nl.y) >> (16 * (k & 1))) & 0xFFFFu);
            uint32_t ax[N];
#pragma unroll
            for (int t = 0; t < N; ++t) ax[t] = (tw[t] >> (8 * k)) & 0xFFu;
            float z;
            const float o = up_pixel<R, FP>(a, rec + lrow * FP + lcol, wt, ax, ay,
                                            (int)((gq >> (8 * k)) & 0xFFu), z);
            ox = k == 0 ? o : ox, oy = k == 1 ? o : oy, oz = k == 2 ? o : oz, ow = k == 3 ? o : ow;
            zx = k == 0 ? z : zx, zy = k == 1 ? z : zy, zz = k == 2 ? z : zz, zw = k == 3 ? z : zw;
        }
        const int64_t oo = (int64_t)Y * a.Wo + xo;
        if (VEC) {
            *reinterpret_cast<float4 *>(a.out + oo) = make_float4(ox, oy, oz, ow);
            if (a.depth) *reinterpret_cast<float4 *>(a.depth + oo) = make_float4(zx, zy, zz, zw);
        } else {
            const float o[4] = {ox, oy, oz, ow}, z[4] = {zx, zy, zz, zw};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (xo + k < a.Wo) {
                    a.out[oo + k] = o[k];
                    if (a.depth) a.depth[oo + k] = z[k];
                }
            }
        }
    }
}

int ufail(const char *msg) { return dsx::set_error(DSX_EINVAL, msg); }

int check_upsample(const dsx_upsample *u) {
    if (!u) return ufail("NULL upsample parameters");
    if (u->type == DSX_UPSAMPLE_NONE) return DSX_OK;
    if (u->type != DSX_UPSAMPLE_JOINT) return ufail("upsample type must be DSX_UPSAMPLE_NONE or DSX_UPSAMPLE_JOINT");
    if (u->radius < 1 || u->radius > 3) return ufail("upsample radius must be in [1, 3]");
    if (u->sigma < dsx::kWmedianMinSigma || u->sigma > dsx::kWmedianMaxSigma) return ufail("upsample sigma must be in [1, 64]");
    if (!std::isfinite(u->max_diff) || !(u->max_diff > 0.0f)) return ufail("upsample max_diff must be finite and > 0");
    return DSX_OK;
}

int64_t first_column(int64_t W, int64_t Wl, int64_t x0) {
    const int64_t num = 2 * W * x0 - Wl;
    return num <= 0 ? 0 : (num + 2 * Wl - 1) / (2 * Wl);
}

template <int R>
void launch(bool vec, dim3 grid, hipStream_t st, const UpArgs &a, const UpTable &t) {
    if (vec) hipLaunchKernelGGL((upsample_joint<R, true>), grid, dim3(kThreads), 0, st, a, t);
    else hipLaunchKernelGGL((upsample_joint<R, false>), grid, dim3(kThreads), 0, st, a, t);
}

}  // namespace

extern "C" {

void dsx_default_upsample(dsx_upsample *u) {
    if (!u) return;
    *u = dsx_upsample{};
    u->type = DSX_UPSAMPLE_JOINT;
    u->radius = 1;
    u->sigma = 8;
    u->max_diff = 1.0f;
}

int dsx_check_upsample(const dsx_upsample *u) {
    dsx::set_error(DSX_OK, "");
    return check_upsample(u);
}

int dsx_upsample_taps(int32_t in_size, int32_t out_size, int32_t radius, int32_t *near, int32_t *tent) {
    dsx::set_error(DSX_OK, "");
    if (in_size < 1 || in_size > kMaxDim || out_size < 1 || out_size > in_size) return ufail("sizes must satisfy 1 <= out_size <= in_size <= 32768");
    if (radius < 1 || radius > 3) return ufail("upsample radius must be in [1, 3]");
    if (!near || !tent) return ufail("NULL array");
    const int64_t I = in_size, O = out_size, r = radius;
    for (int64_t X = 0; X < I; ++X) {
        const int64_t k0 = ((2 * X + 1) * O) / (2 * I);
        near[X] = (int32_t)k0;
        for (int64_t t = 0; t <= 2 * r; ++t) {
            const int64_t k = k0 + t - r;
            int64_t n = (2 * X + 1) * O - (2 * k + 1) * I;
            if (n < 0) n = -n;
            const int64_t q = (64 * n + (r + 1) * I) / (2 * (r + 1) * I);
            tent[X * (2 * r + 1) + t] = (int32_t)(q >= 64 ? 0 : 64 - q);
        }
    }
    return DSX_OK;
}

int32_t dsx_upsample_x0(int32_t W, int32_t Wl, int32_t x0) {
    dsx::set_error(DSX_OK, "");
    if (W < 1 || W > kMaxDim || Wl < 1 || Wl > W || x0 < 0 || x0 > Wl) return ufail("bad W, Wl or x0");
    return (int32_t)first_column(W, Wl, x0);
}

int dsx_upsample_device(const void *d_disp, int32_t h, int32_t w, int64_t in_pitch, int32_t x0, const void *d_guide_lo,
                        int32_t Wl, int64_t guide_lo_stride_bytes, const void *d_guide, int32_t H, int32_t W,
                        int32_t channels, int64_t guide_stride_bytes, const dsx_upsample *params, void *d_out_disp,
                        void *d_out_depth, double focal_length, double baseline, double doffs, double eps,
                        double max_depth, int32_t has_max_depth, void *hip_stream) {
    dsx::set_error(DSX_OK, "");
    if (int rc = check_upsample(params)) return rc;
    if (params->type != DSX_UPSAMPLE_JOINT) return ufail("dsx_upsample_device runs type DSX_UPSAMPLE_JOINT");
    if (h < 1 || w < 0 || x0 < 0 || Wl < 1) return ufail("bad low-resolution shape");
    if (H < 1 || W < 1 || H > kMaxDim || W > kMaxDim) return ufail("bad full-size shape (H, W in [1, 32768])");
    if (h > H) return ufail("h > H: the call does not downscale");
    if (Wl > W) return ufail("Wl > W: the call does not downscale");
    if ((int64_t)x0 + w != Wl) return ufail("the map must cover low-resolution columns x0 .. Wl - 1 (x0 + w == Wl)");
    if (channels != 1 && channels != 3) return ufail("channels must be 1 or 3");
    if (has_max_depth != 0 && has_max_depth != 1) return ufail("has_max_depth must be 0 or 1");
    const int64_t X0 = first_column(W, Wl, x0);
    if (w == 0 || X0 >= W) return DSX_OK;  // nothing to do
    if (!d_disp) return ufail("d_disp is NULL");
    if (!d_guide_lo) return ufail("d_guide_lo is NULL");
    if (!d_guide) return ufail("d_guide is NULL");
    if (!d_out_disp) return ufail("d_out_disp is NULL");
    if (in_pitch < w) return ufail("bad pitch");
    if (guide_lo_stride_bytes < Wl) return ufail("bad low-resolution guide stride");
    if (guide_stride_bytes < (int64_t)W * channels) return ufail("bad guide stride");
    if (d_out_disp == d_disp) return ufail("d_out_disp must not be d_disp (every window reads its neighbours' inputs)");
    if (d_out_depth && (d_out_depth == d_disp || d_out_depth == d_out_disp)) return ufail("d_out_depth must be a buffer of its own");
    UpTable tab;
    if (dsx::wmedian_weights(params->sigma, tab.t) != 0) return ufail("bad sigma");
    UpArgs a{};
    a.d = static_cast<const uint32_t *>(d_disp);
    a.dpitch = in_pitch;
    a.g = static_cast<const uint8_t *>(d_guide_lo);
    a.gstride = guide_lo_stride_bytes;
    a.G = static_cast<const uint8_t *>(d_guide);
    a.Gstride = guide_stride_bytes;
    a.out = static_cast<float *>(d_out_disp);
    a.depth = static_cast<float *>(d_out_depth);
    a.h = h, a.w = w, a.x0 = x0, a.Wl = Wl;
    a.H = H, a.W = W, a.ch = channels;
    a.X0 = (int)X0, a.Wo = W - (int)X0;
    a.max_diff = params->max_diff;
    a.sx = (float)((double)W / (double)Wl);
    a.fB = (float)(focal_length * baseline);  // the depth map's own constant (dsx_api.hip post args)
    a.doffs = (float)doffs, a.eps = (float)eps, a.max_depth = (float)max_depth;
    a.has_max = has_max_depth;
    const auto al16 = [](const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; };
    const bool vec = (a.Wo & 3) == 0 && al16(d_out_disp) && al16(d_out_depth);
    const dim3 grid((a.Wo + kTW - 1) / kTW, (H + kTH - 1) / kTH);
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if (params->radius == 1) launch<1>(vec, grid, st, a, tab);
    else if (params->radius == 2) launch<2>(vec, grid, st, a, tab);
    else launch<3>(vec, grid, st, a, tab);
    if (hipError_t e = hipGetLastError())
        return dsx::set_error(DSX_EHIP, std::string("upsample_joint: ") + hipGetErrorString(e));
    return DSX_OK;
}

}  // extern "C"
