// Area downscale on the device: the input step of depthlib/input.py:38-43,63-67 and
// depthlib/threaded_stereo.py:45-47 (cv2.resize INTER_AREA), in the arithmetic of this project's host
// step depthestimation_amd/input.py resize_area, which is Pillow's BOX resampling - bit for bit:
//
//   per axis, input size I, output size O:  scale = I / O, fs = max(scale, 1), sup = fs / 2, ss = 1 / fs
//   output o:  c = (o + 0.5) scale;  taps x in [int(c - sup + 0.5), int(c + sup + 0.5)) clipped to the
//              axis with -0.5 < (x - c + 0.5) ss <= 0.5 (n of them, contiguous);  k = int(2^22 / n + 0.5)
//              out = min(255, (2^21 + k * sum of the taps) >> 22)
//   the horizontal pass runs first and rounds to u8, the vertical pass runs on those u8 values.
//
// The double arithmetic runs once per shape on the host (resize_area_table below, the one C home of the
// rule); the kernels see (start, count, k) per output column and per output row and use 32-bit integers
// only (255 n k + 2^21 < 2^31), so nothing depends on the device's floating point.
//
// One kernel, one launch per image, each source byte read once (the windows of different outputs are
// disjoint): resize_area, one lane per output pixel, a 64 x 4 pixel tile per block.  The lane walks its
// window row by row and tap by tap with byte loads (windows of at most 2 x 2 taps, i.e. factors from 0.5
// up: all taps loaded before the first is used), the three channels of a tap at immediate offsets of
// one address; per row it rounds each channel's horizontal sum to u8 and adds it to that channel's
// vertical sum, after the last row it applies the vertical (k, >> 22) and stores the C bytes, or with the
// fused gray output the one byte of dsx_rectify.hip's gray formula on the three rounded values, as
// to_grayscale_bgr(resize_area(img)) does.  Neighbouring lanes read neighbouring windows, so a wave's
// loads of one tap fall into the same few cache lines.  At the sizes of this path (a 1080p frame is
// 6.2 MB) the kernel is bound by instruction issue and the launch, not by HBM: DESIGN.md 4.3, where the
// LDS-strip form that was measured against it is recorded too.
#include "dsx_internal.h"

#include <mutex>
#include <vector>

namespace dsx {

#pragma clang fp contract(off)

int resize_area_table(int in_size, int out_size, int32_t *start, int32_t *count, int32_t *coef) {
    if (out_size < 1 || out_size > in_size || !start || !count || !coef) return -1;
    const volatile double scale = (double)in_size / (double)out_size;
    const volatile double fs = scale < 1.0 ? 1.0 : scale;
    const volatile double sup = 0.5 * fs;
    const volatile double ss = 1.0 / fs;
    for (int o = 0; o < out_size; ++o) {
        const volatile double c = ((double)o + 0.5) * scale;
        const volatile double lo = c - sup;
        const volatile double hi = c + sup;
        int xmin = (int)(lo + 0.5), xmax = (int)(hi + 0.5);
        if (xmin < 0) xmin = 0;
        if (xmax > in_size) xmax = in_size;
        int first = -1, n = 0;
        for (int x = xmin; x < xmax; ++x) {
            const volatile double d = (double)x - c;
            const volatile double w = (d + 0.5) * ss;
            if (w > -0.5 && w <= 0.5) {
                if (first < 0) first = x;
                ++n;
            }
        }
        start[o] = first < 0 ? xmin : first;
        count[o] = n;
        const volatile double inv = n > 0 ? 1.0 / (double)n : 0.0;
        coef[o] = n > 0 ? (int32_t)(inv * 4194304.0 + 0.5) : 0;
    }
    return 0;
}

namespace {

constexpr int kThreads = 256;

struct ResizeArgs {
    const uint8_t *img;  // Hs x Ws x C, row stride in bytes
    int64_t stride;
    int Ho, Wo;
    const int32_t *htab;  // start[Wo], count[Wo], coef[Wo]
    const int32_t *vtab;  // start[Ho], count[Ho], coef[Ho]
    uint8_t *out;         // Ho x Wo x C, or Ho x Wo gray
    int64_t out_stride;
};

__device__ __forceinline__ uint32_t round22(uint32_t k, uint32_t sum) {
    const uint32_t v = (k * sum + (1u << 21)) >> 22;
    return v > 255u ? 255u : v;
}

__device__ __forceinline__ uint32_t gray3(uint32_t c0, uint32_t c1, uint32_t c2) {
    return (c0 * 1868u + c1 * 9617u + c2 * 4899u + (1u << 13)) >> 14;  // gray_at, dsx_rectify.hip
}

// MT > 0: every window has 1 .. MT taps per axis (factors from 0.5 up: MT = 2).  The MT x MT taps are then
// loaded before the first is used - one memory round instead of one per tap - from addresses clamped
// into the window, and the taps past a window's count drop out of the sums.  MT = 0: any window, by loops.
template <int C, bool GRAY, int MT>
__global__ __launch_bounds__(kThreads) void resize_area(ResizeArgs a) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= a.Wo || y >= a.Ho) return;
    const int hs = a.htab[x], hn = a.htab[a.Wo + x];
    const uint32_t hk = (uint32_t)a.htab[2 * a.Wo + x];
    const int vs = a.vtab[y], vn = a.vtab[a.Ho + y];
    const uint32_t vk = (uint32_t)a.vtab[2 * a.Ho + y];
    uint32_t vsum[C];
#pragma unroll
    for (int c = 0; c < C; ++c) vsum[c] = 0;
    const uint8_t *row = a.img + (int64_t)vs * a.stride + (int64_t)hs * C;
    if constexpr (MT > 0) {
        uint32_t tap[MT][MT][C];
#pragma unroll
        for (int j = 0; j < MT; ++j) {
            const uint8_t *r = row + (j < vn ? j : vn - 1) * a.stride;
#pragma unroll
            for (int t = 0; t < MT; ++t) {
                const uint8_t *p = r + (t < hn ? t : hn - 1) * C;
#pragma unroll
                for (int c = 0; c < C; ++c) tap[j][t][c] = p[c];
            }
        }
#pragma unroll
        for (int j = 0; j < MT; ++j) {
#pragma unroll
            for (int c = 0; c < C; ++c) {
                uint32_t sum = 0;
#pragma unroll
                for (int t = 0; t < MT; ++t) sum += t < hn ? tap[j][t][c] : 0u;
                vsum[c] += j < vn ? round22(hk, sum) : 0u;
            }
        }
    } else {
        for (int j = 0; j < vn; ++j, row += a.stride) {
            uint32_t sum[C];
#pragma unroll
            for (int c = 0; c < C; ++c) sum[c] = 0;
            const uint8_t *p = row;
            for (int t = 0; t < hn; ++t, p += C) {
#pragma unroll
                for (int c = 0; c < C; ++c) sum[c] += p[c];
            }
#pragma unroll
            for (int c = 0; c < C; ++c) vsum[c] += round22(hk, sum[c]);
        }
    }
    uint32_t v[C];
#pragma unroll
    for (int c = 0; c < C; ++c) v[c] = round22(vk, vsum[c]);
    uint8_t *o = a.out + (int64_t)y * a.out_stride;
    if constexpr (GRAY) {
        o[x] = (uint8_t)gray3(v[0], v[1], v[2]);
    } else {
#pragma unroll
        for (int c = 0; c < C; ++c) o[(int64_t)x * C + c] = (uint8_t)v[c];
    }
}

// The two tables of one (Hs, Ws, Ho, Wo) on one device, resident until evicted or dsx_shutdown.
struct TableEntry {
    int dev, Hs, Ws, Ho, Wo;
    int32_t *d_tab = nullptr;    // htab (3 Wo) then vtab (3 Ho)
    std::vector<int32_t> h_tab;  // the upload's source, kept with the entry
    bool small = false;          // every window of both axes has 1 or 2 taps (kernel form MT = 2)
    uint64_t used = 0;           // LRU stamp
};

constexpr int kMaxTablesPerDevice = 8;
std::mutex g_tab_mu;
std::vector<TableEntry> g_tabs;
uint64_t g_tab_clock = 0;

// g_tab_mu held.  The entry of (dev, shape), built and uploaded on `st` on first use.
hipError_t get_tables(int dev, int Hs, int Ws, int Ho, int Wo, hipStream_t st, TableEntry **out) {
    for (auto &t : g_tabs)
        if (t.dev == dev && t.Hs == Hs && t.Ws == Ws && t.Ho == Ho && t.Wo == Wo) {
            t.used = ++g_tab_clock;
            *out = &t;
            return hipSuccess;
        }
    // bounded per device: drop the least recently used (hipFree waits for the device, so a kernel
    // still reading the table on another stream finishes first)
    int n = 0, lru = -1;
    for (size_t i = 0; i < g_tabs.size(); ++i)
        if (g_tabs[i].dev == dev) {
            ++n;
            if (lru < 0 || g_tabs[i].used < g_tabs[lru].used) lru = (int)i;
        }
    if (n >= kMaxTablesPerDevice) {
        (void)hipFree(g_tabs[lru].d_tab);
        g_tabs.erase(g_tabs.begin() + lru);
    }
    TableEntry t;
    t.dev = dev;
    t.Hs = Hs;
    t.Ws = Ws;
    t.Ho = Ho;
    t.Wo = Wo;
    t.h_tab.resize(3 * ((size_t)Wo + Ho));
    int32_t *h = t.h_tab.data(), *v = h + 3 * (size_t)Wo;
    if (resize_area_table(Ws, Wo, h, h + Wo, h + 2 * (size_t)Wo) != 0 ||
        resize_area_table(Hs, Ho, v, v + Ho, v + 2 * (size_t)Ho) != 0)
        return hipErrorInvalidValue;
    t.small = true;
    for (int x = 0; x < Wo; ++x) t.small = t.small && h[Wo + x] >= 1 && h[Wo + x] <= 2;
    for (int y = 0; y < Ho; ++y) t.small = t.small && v[Ho + y] >= 1 && v[Ho + y] <= 2;
    const size_t bytes = t.h_tab.size() * sizeof(int32_t);
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&t.d_tab), bytes);
    if (e != hipSuccess) return e;
    // on the call's stream, and complete before any stream may launch with it (first use only)
    e = hipMemcpyAsync(t.d_tab, t.h_tab.data(), bytes, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        (void)hipFree(t.d_tab);
        return e;
    }
    t.used = ++g_tab_clock;
    g_tabs.push_back(std::move(t));
    *out = &g_tabs.back();
    return hipSuccess;
}

template <int C, bool GRAY>
hipError_t launch_one(const ResizeArgs &a, bool small, hipStream_t st) {
    const dim3 grid((a.Wo + 63) / 64, (a.Ho + 3) / 4);
    if (small) hipLaunchKernelGGL((resize_area<C, GRAY, 2>), grid, dim3(kThreads), 0, st, a);
    else hipLaunchKernelGGL((resize_area<C, GRAY, 0>), grid, dim3(kThreads), 0, st, a);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_resize_area(const uint8_t *img, int64_t stride, int Hs, int Ws, int channels, int Ho, int Wo,
                              bool gray, uint8_t *out, int64_t out_stride, hipStream_t st) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    // the launch stays under the lock: an eviction by another thread must not free the table between
    // the lookup and the launch
    std::lock_guard<std::mutex> lk(g_tab_mu);
    TableEntry *t = nullptr;
    e = get_tables(dev, Hs, Ws, Ho, Wo, st, &t);
    if (e != hipSuccess) return e;
    ResizeArgs a{};
    a.img = img;
    a.stride = stride;
    a.Ho = Ho;
    a.Wo = Wo;
    a.htab = t->d_tab;
    a.vtab = t->d_tab + 3 * (size_t)Wo;
    a.out = out;
    a.out_stride = out_stride;
    if (channels == 1) return launch_one<1, false>(a, t->small, st);
    return gray ? launch_one<3, true>(a, t->small, st) : launch_one<3, false>(a, t->small, st);
}

bool resize_has_tables() {
    std::lock_guard<std::mutex> lk(g_tab_mu);
    return !g_tabs.empty();
}

void resize_forget_all() {
    std::lock_guard<std::mutex> lk(g_tab_mu);
    int prev = 0;
    (void)hipGetDevice(&prev);
    for (auto &t : g_tabs)
        if (hipSetDevice(t.dev) == hipSuccess) (void)hipFree(t.d_tab);
    (void)hipSetDevice(prev);
    g_tabs.clear();
}

}  // namespace dsx
