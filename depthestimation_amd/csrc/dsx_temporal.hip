// Temporal disparity filter (dsx_temporal_params / dsx_tfilter of dsx.h; host restatement
// depthestimation_amd/temporal.py): a motion-gated recursive average of the finished disparity map with a
// temporal hole filler.  Per pixel, all in float32, every operation correctly rounded and uncontracted:
//
//   v = 0 < d < inf;  M = box sum (radius r, replicate clamp) of |G - P|;  static = prev && M <= thr (2r+1)^2
//   v && static && n > 0 && |d - S| <= max_diff:  S' = S + (d - S) A[n], n' = min(n + 1, max_age), h' = 0, out = S'
//   else v:                                       S' = d, n' = 1, h' = 0, out = d
//   else static && n > 0 && h < hold:             out = S, S and n kept, h' = h + 1
//   else:                                         out = d, S' = 0, n' = 0, h' = 0
//   P <- G
//
// One launch per frame, a streaming kernel of about 27 B per pixel (read d 4, S 4, G 1, P 1, n + h 2; write out
// 4, S 4, P 1, n + h 2, depth 4).  A block of 256 threads owns a tile of kTW x kTH = 256 x 8 pixels; a lane owns
// 4 consecutive pixels of a row (a wave covers one 256-pixel row segment: 1 KiB of each float plane per
// instruction on the 16-byte path) and two rows, 4 apart.
//   temporal_step<R, VEC>
//     R > 0:  |G - P| is computed ONCE per pixel into an LDS byte tile of (kTH + 2R) rows x (kTW + 8) columns -
//             a halo of one dword either side, of which R bytes are read - each thread filling dwords: a dword
//             whose 4 columns are inside the image reads G with one (unaligned) dword load and P with an aligned
//             one; dwords that touch the image's edge clamp byte by byte.  The box sum of a pixel is then
//             v_sad_u8 against 0 of the (2R+1)-byte window, cut from 3 consecutive tile dwords by v_alignbyte:
//             R = 1: one SAD per row and pixel (3 bytes masked), R = 2: one SAD plus one byte.
//     R == 0: M = |G - P| of the pixel itself: no LDS, no barrier.
//     VEC:    d, out and depth rows are 16-byte aligned: float4 loads and stores.  Otherwise the caller's planes
//             are read and written pixel by pixel.  The filter's own planes (S, n, h, P) have pitches that are
//             multiples of 4 pixels and are read and written as float4 / dwords on both paths.
// P is double-buffered (the window reads the neighbours' P while this frame's G becomes the next P); the parity
// lives in the filter object.  S, n and h are updated in place.  No atomics, no block waits on another, no
// cooperative launch, no scratch (the gains are gathered from a 65-float device table, never indexed in
// registers).  The first frame after a reset runs with prev = 0: the state planes are not read, so a reset is
// no device work.
#include "dsx_internal.h"

#include <cmath>
#include <string>

#include "../../include/dsx.h"

namespace dsx {
int set_error(int code, const std::string &msg);  // dsx_api.hip: the message behind dsx_last_error
}

struct dsx_tfilter {
    int device = 0;
    dsx_temporal_params p{};
    float gains[65] = {};
    float *dGains = nullptr;       // 65 floats
    float *S = nullptr;            // H x Wp
    uint8_t *n = nullptr, *h = nullptr;  // H x Wp
    uint8_t *P[2] = {nullptr, nullptr};  // H x Wp each
    int cur = 0;                   // P[cur] holds the previous frame's guide
    int32_t H = 0, W = 0;
    int64_t Wp = 0;                // pitch of the state planes, a multiple of 4
    int64_t bytes = 0;
    bool prev = false;
    hipEvent_t done = nullptr;
    hipStream_t lastStream = nullptr;
    bool pending = false;
};

namespace {

constexpr int kTW = DSX_TEMPORAL_TILE_W, kTH = DSX_TEMPORAL_TILE_H, kThreads = 256;
constexpr int kRowsPerThread = kTH / (kThreads / 64);
constexpr int kTileDwords = kTW / 4 + 2;  // one halo dword either side
static_assert(kTW == 64 * 4, "a wave covers one row segment of the tile, 4 pixels per lane");
static_assert(kTH % (kThreads / 64) == 0, "every wave owns whole rows");

struct TemporalArgs {
    const float *d;
    int64_t dpitch;  // elements
    const uint8_t *G;
    int64_t gstride;  // bytes
    float *out, *depth;  // contiguous H x W (depth may be null)
    float *S;
    uint8_t *n, *h;
    const uint8_t *P;  // previous guide
    uint8_t *Pn;       // next guide
    int64_t Wp;
    const float *gains;
    int H, W;
    int prev;
    int max_age, hold, mthr;  // mthr = motion_threshold * (2r + 1)^2
    float max_diff;
    float fB, doffs, eps, max_depth;
    int has_max;
};

__device__ __forceinline__ uint32_t load_u32(const uint8_t *p) {  // any alignment
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}

// |a - b| of each of the 4 bytes
__device__ __forceinline__ uint32_t absdiff_u8x4(uint32_t a, uint32_t b) {
    uint32_t r = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        r |= __builtin_amdgcn_sad_u8((a >> (8 * k)) & 0xFFu, (b >> (8 * k)) & 0xFFu, 0u) << (8 * k);
    return r;
}

#pragma clang fp contract(off)

// one pixel of the rule; returns out and updates S, n, h
__device__ __forceinline__ float temporal_pixel(const TemporalArgs &a, float d, bool stat, float &S, uint32_t &n,
                                                uint32_t &h) {
    const bool v = d > 0.0f && d < __builtin_inff();
    const bool have = stat && n > 0;
    const float diff = d - S;
    const float gain = a.gains[n];  // n <= max_age <= 64; entry 0 is 0
    if (v && have && __builtin_fabsf(diff) <= a.max_diff) {
        S = S + diff * gain;
        n = min(n + 1u, (uint32_t)a.max_age);
        h = 0;
        return S;
    }
    if (v) {
        S = d, n = 1, h = 0;
        return d;
    }
    if (have && h < (uint32_t)a.hold) {
        h = h + 1;
        return S;
    }
    S = 0.0f, n = 0, h = 0;
    return d;
}

__device__ __forceinline__ float temporal_depth(const TemporalArgs &a, float o) {
    const float adj = o + a.doffs;
    float z = adj > a.eps ? __fdiv_rn(a.fB, adj) : __builtin_inff();
    if (a.has_max && z > a.max_depth) z = a.max_depth;
    return z;
}

#pragma clang fp contract(on)

template <int R, bool VEC>
__global__ __launch_bounds__(kThreads) void temporal_step(TemporalArgs a) {
    static_assert(R >= 0 && R <= 2, "motion_radius 0..2");
    __shared__ uint32_t ad[R > 0 ? (kTH + 2 * R) * kTileDwords : 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int x0 = blockIdx.x * kTW, y0 = blockIdx.y * kTH;
    const bool prev = a.prev != 0;  // uniform
    if (R > 0 && prev) {
        // tile dword k of tile row ty holds |G - P| of columns x0 - 4 + 4k .. + 3 of row cy(y0 + ty - R)
        for (int q = tid; q < (kTH + 2 * R) * kTileDwords; q += kThreads) {
            const int ty = q / kTileDwords, k = q - ty * kTileDwords;
            const int y = min(max(y0 + ty - R, 0), a.H - 1);
            const int xb = x0 - 4 + 4 * k;
            const uint8_t *g = a.G + (int64_t)y * a.gstride;
            const uint8_t *p = a.P + (int64_t)y * a.Wp;
            uint32_t gv, pv;
            if (xb >= 0 && xb + 3 < a.W) {
                gv = load_u32(g + xb);
                pv = *reinterpret_cast<const uint32_t *>(p + xb);
            } else {
                gv = pv = 0;
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const int x = min(max(xb + b, 0), a.W - 1);
                    gv |= (uint32_t)g[x] << (8 * b);
                    pv |= (uint32_t)p[x] << (8 * b);
                }
            }
            ad[q] = absdiff_u8x4(gv, pv);
        }
        __syncthreads();
    }
    const int x = x0 + 4 * lane;
    if (x >= a.W) return;
    const bool whole = x + 3 < a.W;  // VEC: always (W is a multiple of 4)
#pragma unroll
    for (int it = 0; it < kRowsPerThread; ++it) {
        const int ty = wave + it * (kThreads / 64), y = y0 + ty;
        if (y >= a.H) break;
        // the frame's guide at the lane's pixels (the next P), and the motion sums
        const uint8_t *g = a.G + (int64_t)y * a.gstride + x;
        uint32_t gv = 0;
        if (whole) {
            gv = load_u32(g);
        } else {
            for (int b = 0; b < a.W - x; ++b) gv |= (uint32_t)g[b] << (8 * b);
        }
        const int64_t so = (int64_t)y * a.Wp + x;
        uint32_t M[4] = {0, 0, 0, 0};
        if (prev) {
            if (R == 0) {
                const uint32_t dv = absdiff_u8x4(gv, *reinterpret_cast<const uint32_t *>(a.P + so));
#pragma unroll
                for (int k = 0; k < 4; ++k) M[k] = (dv >> (8 * k)) & 0xFFu;
            } else {
#pragma unroll
                for (int j = 0; j <= 2 * R; ++j) {
                    const uint32_t *row = ad + (ty + j) * kTileDwords + lane;
                    const uint32_t w[3] = {row[0], row[1], row[2]};  // columns x - 4 .. x + 7
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int s = 4 - R + k;  // first byte of pixel k's window in the 12-byte string
                        uint32_t win = (s & 3) ? __builtin_amdgcn_alignbyte(w[(s >> 2) + 1], w[s >> 2], s & 3) : w[s >> 2];
                        if (R == 1) win &= 0x00FFFFFFu;
                        M[k] = __builtin_amdgcn_sad_u8(win, 0u, M[k]);
                        if (R == 2) M[k] += (w[(s + 4) >> 2] >> (8 * ((s + 4) & 3))) & 0xFFu;
                    }
                }
            }
        }
        // state
        float S[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        uint32_t nv = 0, hv = 0;
        if (prev) {
            const float4 s4 = *reinterpret_cast<const float4 *>(a.S + so);
            S[0] = s4.x, S[1] = s4.y, S[2] = s4.z, S[3] = s4.w;
            nv = *reinterpret_cast<const uint32_t *>(a.n + so);
            hv = *reinterpret_cast<const uint32_t *>(a.h + so);
        }
        // the frame's map
        float d[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        const float *dp = a.d + (int64_t)y * a.dpitch + x;
        if (VEC) {
            const float4 d4 = *reinterpret_cast<const float4 *>(dp);
            d[0] = d4.x, d[1] = d4.y, d[2] = d4.z, d[3] = d4.w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (x + k < a.W) d[k] = dp[k];
        }
        float o[4], z[4];
        uint32_t nn = 0, hn = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            uint32_t n1 = (nv >> (8 * k)) & 0xFFu, h1 = (hv >> (8 * k)) & 0xFFu;
            o[k] = temporal_pixel(a, d[k], prev && M[k] <= (uint32_t)a.mthr, S[k], n1, h1);
            z[k] = temporal_depth(a, o[k]);
            nn |= n1 << (8 * k);
            hn |= h1 << (8 * k);
        }
        *reinterpret_cast<float4 *>(a.S + so) = make_float4(S[0], S[1], S[2], S[3]);
        *reinterpret_cast<uint32_t *>(a.n + so) = nn;
        *reinterpret_cast<uint32_t *>(a.h + so) = hn;
        *reinterpret_cast<uint32_t *>(a.Pn + so) = gv;
        const int64_t oo = (int64_t)y * a.W + x;
        if (VEC) {
            *reinterpret_cast<float4 *>(a.out + oo) = make_float4(o[0], o[1], o[2], o[3]);
            if (a.depth) *reinterpret_cast<float4 *>(a.depth + oo) = make_float4(z[0], z[1], z[2], z[3]);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (x + k < a.W) {
                    a.out[oo + k] = o[k];
                    if (a.depth) a.depth[oo + k] = z[k];
                }
            }
        }
    }
}

int tfail(const char *msg) { return dsx::set_error(DSX_EINVAL, msg); }

int hip_fail(const char *what, hipError_t e) {
    return dsx::set_error(e == hipErrorOutOfMemory ? DSX_ENOMEM : DSX_EHIP, std::string(what) + ": " + hipGetErrorString(e));
}

int check_temporal(const dsx_temporal_params *t) {
    if (!t) return tfail("NULL temporal parameters");
    if (t->type == DSX_TEMPORAL_NONE) return DSX_OK;
    if (t->type != DSX_TEMPORAL_RECURSIVE) return tfail("temporal type must be DSX_TEMPORAL_NONE or DSX_TEMPORAL_RECURSIVE");
    if (t->max_age < 1 || t->max_age > 64) return tfail("temporal max_age must be in [1, 64]");
    if (!std::isfinite(t->max_diff) || !(t->max_diff > 0.0f)) return tfail("temporal max_diff must be finite and > 0");
    if (t->motion_radius < 0 || t->motion_radius > 2) return tfail("temporal motion_radius must be in [0, 2]");
    if (t->motion_threshold < 0 || t->motion_threshold > 255) return tfail("temporal motion_threshold must be in [0, 255]");
    if (t->hold < 0 || t->hold > 255) return tfail("temporal hold must be in [0, 255]");
    return DSX_OK;
}

void free_state(dsx_tfilter *f) {
    (void)hipFree(f->S);
    (void)hipFree(f->n);
    (void)hipFree(f->h);
    (void)hipFree(f->P[0]);
    (void)hipFree(f->P[1]);
    f->S = nullptr, f->n = f->h = f->P[0] = f->P[1] = nullptr;
    f->H = f->W = 0, f->Wp = 0, f->bytes = 0, f->prev = false;
}

// waits until the filter's last launch has finished (before its buffers are freed or its table rewritten)
int wait_done(dsx_tfilter *f) {
    if (f->pending) {
        if (hipError_t e = hipEventSynchronize(f->done)) return hip_fail("hipEventSynchronize", e);
        f->pending = false;
    }
    return DSX_OK;
}

int upload_gains(dsx_tfilter *f) {
    if (hipError_t e = hipMemcpy(f->dGains, f->gains, sizeof(f->gains), hipMemcpyHostToDevice)) return hip_fail("hipMemcpy", e);
    return DSX_OK;
}

void fill_gains(dsx_tfilter *f) {
    for (float &g : f->gains) g = 0.0f;
    dsx_temporal_gains(64, f->gains);  // every age: the table does not depend on max_age
}

template <int R>
void launch(bool vec, dim3 grid, hipStream_t st, const TemporalArgs &a) {
    if (vec) hipLaunchKernelGGL((temporal_step<R, true>), grid, dim3(kThreads), 0, st, a);
    else hipLaunchKernelGGL((temporal_step<R, false>), grid, dim3(kThreads), 0, st, a);
}

}  // namespace

extern "C" {

void dsx_default_temporal(dsx_temporal_params *t) {
    if (!t) return;
    *t = dsx_temporal_params{};
    t->type = DSX_TEMPORAL_RECURSIVE;
    t->max_age = 4;
    t->max_diff = 1.0f;
    t->motion_radius = 1;
    t->motion_threshold = 6;
    t->hold = 2;
}

int dsx_check_temporal(const dsx_temporal_params *t) {
    dsx::set_error(DSX_OK, "");
    return check_temporal(t);
}

int dsx_temporal_gains(int32_t max_age, float *out) {
    dsx::set_error(DSX_OK, "");
    if (max_age < 1 || max_age > 64) return tfail("temporal max_age must be in [1, 64]");
    if (!out) return tfail("NULL gains array");
    out[0] = 0.0f;
    for (int n = 1; n <= max_age; ++n) out[n] = (float)(1.0 / (double)(n + 1));
    return max_age + 1;
}

int dsx_tfilter_create(int device, const dsx_temporal_params *t, dsx_tfilter **out) {
    dsx::set_error(DSX_OK, "");
    if (!out) return tfail("NULL output");
    *out = nullptr;
    if (int rc = check_temporal(t)) return rc;
    if (t->type != DSX_TEMPORAL_RECURSIVE) return tfail("a filter object needs type DSX_TEMPORAL_RECURSIVE");
    if (device < 0) return tfail("bad device");
    if (hipError_t e = hipSetDevice(device)) return hip_fail("hipSetDevice", e);
    int wave = 0;  // a lane owns 4 pixels and a wave one 256-pixel row segment: wave size 64 is assumed
    if (hipError_t e = hipDeviceGetAttribute(&wave, hipDeviceAttributeWarpSize, device)) return hip_fail("hipDeviceGetAttribute", e);
    if (wave != 64) return dsx::set_error(DSX_EHIP, "the temporal filter needs a device of wave size 64");
    dsx_tfilter *f = new dsx_tfilter();
    f->device = device;
    f->p = *t;
    fill_gains(f);
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&f->dGains), sizeof(f->gains));
    if (e == hipSuccess) e = hipEventCreateWithFlags(&f->done, hipEventDisableTiming);
    if (e != hipSuccess) {
        (void)hipFree(f->dGains);
        delete f;
        return hip_fail("dsx_tfilter_create", e);
    }
    if (int rc = upload_gains(f)) {
        (void)hipEventDestroy(f->done);
        (void)hipFree(f->dGains);
        delete f;
        return rc;
    }
    *out = f;
    return DSX_OK;
}

int dsx_tfilter_set_params(dsx_tfilter *f, const dsx_temporal_params *t) {
    dsx::set_error(DSX_OK, "");
    if (!f) return tfail("NULL filter");
    if (int rc = check_temporal(t)) return rc;
    if (t->type != DSX_TEMPORAL_RECURSIVE) return tfail("a filter object needs type DSX_TEMPORAL_RECURSIVE");
    if (hipError_t e = hipSetDevice(f->device)) return hip_fail("hipSetDevice", e);
    if (int rc = wait_done(f)) return rc;
    f->p = *t;
    f->prev = false;
    return DSX_OK;
}

int dsx_tfilter_reset(dsx_tfilter *f) {
    dsx::set_error(DSX_OK, "");
    if (!f) return tfail("NULL filter");
    f->prev = false;
    return DSX_OK;
}

int dsx_tfilter_bytes(dsx_tfilter *f, int64_t *bytes) {
    dsx::set_error(DSX_OK, "");
    if (!f || !bytes) return tfail("NULL argument");
    *bytes = f->bytes + (int64_t)sizeof(f->gains);
    return DSX_OK;
}

int dsx_tfilter_destroy(dsx_tfilter *f) {
    dsx::set_error(DSX_OK, "");
    if (!f) return DSX_OK;
    (void)hipSetDevice(f->device);
    (void)wait_done(f);
    free_state(f);
    (void)hipFree(f->dGains);
    if (f->done) (void)hipEventDestroy(f->done);
    delete f;
    return DSX_OK;
}

int dsx_tfilter_run_device(dsx_tfilter *f, const void *d_disp, int32_t H, int32_t W, int64_t in_pitch,
                           const void *d_guide, int64_t guide_stride_bytes, void *d_out_disp, void *d_out_depth,
                           double focal_length, double baseline, double doffs, double eps, double max_depth,
                           int32_t has_max_depth, void *hip_stream) {
    dsx::set_error(DSX_OK, "");
    // the arguments first, the filter last: every argument error is reported without a filter or a device
    if (H < 0 || W < 0) return tfail("bad shape");
    if (H == 0 || W == 0) return f ? DSX_OK : tfail("NULL filter");
    if (!d_disp) return tfail("d_disp is NULL");
    if (!d_guide) return tfail("d_guide is NULL");
    if (!d_out_disp) return tfail("d_out_disp is NULL");
    if (in_pitch < W) return tfail("bad pitch");
    if (guide_stride_bytes < W) return tfail("bad guide stride");
    if (H > kTH * 65535) return tfail("image too tall (H <= 524280)");
    if (has_max_depth != 0 && has_max_depth != 1) return tfail("has_max_depth must be 0 or 1");
    if (d_out_disp == d_disp && in_pitch != W) return tfail("in place needs in_pitch == W");
    if (d_out_depth && (d_out_depth == d_disp || d_out_depth == d_out_disp)) return tfail("d_out_depth must be a buffer of its own");
    if (!f) return tfail("NULL filter");
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if (hipError_t e = hipSetDevice(f->device)) return hip_fail("hipSetDevice", e);
    if (H != f->H || W != f->W) {
        // a shape change: wait for the last launch, reallocate, reset
        if (int rc = wait_done(f)) return rc;
        free_state(f);
        const int64_t Wp = ((int64_t)W + 3) & ~(int64_t)3, np = (int64_t)H * Wp;
        hipError_t e = hipMalloc(reinterpret_cast<void **>(&f->S), np * sizeof(float));
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&f->n), np);
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&f->h), np);
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&f->P[0]), np);
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&f->P[1]), np);
        if (e != hipSuccess) {
            free_state(f);
            return hip_fail("temporal state", e);
        }
        f->H = H, f->W = W, f->Wp = Wp, f->bytes = np * 8, f->cur = 0;
    }
    if (f->pending && f->lastStream != st) {
        if (hipError_t e = hipStreamWaitEvent(st, f->done, 0)) return hip_fail("hipStreamWaitEvent", e);
    }
    TemporalArgs a{};
    a.d = static_cast<const float *>(d_disp);
    a.dpitch = in_pitch;
    a.G = static_cast<const uint8_t *>(d_guide);
    a.gstride = guide_stride_bytes;
    a.out = static_cast<float *>(d_out_disp);
    a.depth = static_cast<float *>(d_out_depth);
    a.S = f->S, a.n = f->n, a.h = f->h;
    a.P = f->P[f->cur], a.Pn = f->P[f->cur ^ 1];
    a.Wp = f->Wp;
    a.gains = f->dGains;
    a.H = H, a.W = W;
    a.prev = f->prev ? 1 : 0;
    const int r = f->p.motion_radius;
    a.max_age = f->p.max_age, a.hold = f->p.hold, a.mthr = f->p.motion_threshold * (2 * r + 1) * (2 * r + 1);
    a.max_diff = f->p.max_diff;
    a.fB = (float)(focal_length * baseline);  // the depth map's own constant (dsx_api.hip post args)
    a.doffs = (float)doffs, a.eps = (float)eps, a.max_depth = (float)max_depth;
    a.has_max = has_max_depth;
    const auto al16 = [](const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; };
    const bool vec = (W & 3) == 0 && (in_pitch & 3) == 0 && al16(d_disp) && al16(d_out_disp) && al16(d_out_depth);
    const dim3 grid((W + kTW - 1) / kTW, (H + kTH - 1) / kTH);
    if (r == 0) launch<0>(vec, grid, st, a);
    else if (r == 1) launch<1>(vec, grid, st, a);
    else launch<2>(vec, grid, st, a);
    if (hipError_t e = hipGetLastError()) return hip_fail("temporal_step", e);
    if (hipError_t e = hipEventRecord(f->done, st)) return hip_fail("hipEventRecord", e);
    f->pending = true;
    f->lastStream = st;
    f->cur ^= 1;
    f->prev = true;
    return DSX_OK;
}

}  // extern "C"
