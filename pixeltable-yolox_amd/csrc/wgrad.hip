// yxh_conv_wgrad: descriptor validation, the tile-id table of the six weight-gradient kernel
// families and its router, and the fixed-order sum of the per-split partials.
#include <cstdlib>

#include "train_common.hpp"
#include "wgrad.hpp"

namespace yxh {

// dW[i] += sum over the splits of ws[split][i], in split order (deterministic)
__global__ __launch_bounds__(256) void wgrad_reduce(const float* ws, int splits, long long ne, float* dw) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= ne) return;
    float s = 0.0f;
    for (int k = 0; k < splits; ++k) s += ws[(long long)k * ne + i];
    dw[i] += s;
}

int ws_reduce(const WgradParams& p, long long splits, hipStream_t st) {
    if (!p.ws) return YXH_OK;
    const long long ne = (long long)p.cout * p.cin_store * p.kh * p.kw;
    hipLaunchKernelGGL(wgrad_reduce, dim3((unsigned)((ne + 255) / 256)), dim3(256), 0, st, (const float*)p.ws,
                       (int)splits, ne, p.dw);
    YXH_CHECK_LAUNCH("wgrad_reduce");
    return YXH_OK;
}

// The weight gradients run on a side stream beside the data-gradient chain; a grid that fills every
// CU's registers leaves the main stream's BatchNorm reductions no room until its blocks retire.
int wgrad_target_blocks() {
    static const int v = [] {
        const char* e = getenv("YXH_WGRAD_BLOCKS");
        const int x = e ? atoi(e) : 512;
        return x < 64 ? 64 : x > 4096 ? 4096 : x;
    }();
    return v;
}

namespace {

// The wgrad tile-id space (yxh_wgrad_desc.tile): one row per kernel family, its contiguous public
// ids, the operand types it is built for and whether it needs a 3x3 pad-1 conv of stride 1 or 2
// (all nine taps per block).  What one family alone asks for (16-byte channel chunks, tile 27's
// stride, conv_wgrad9's single plain source) stays in that family's dispatch.
enum : unsigned { WG_F32 = 1u, WG_16BIT = 2u, WG_ANY = WG_F32 | WG_16BIT };

struct WgradFamily {
    const char* name;
    int first, last;  // public ids
    unsigned dtypes;  // WG_*
    bool nine_tap;    // 3x3, pad 1, stride 1 or 2 only
    int (*fn)(int dtype, int tile, const WgradParams& p, hipStream_t st);
};

constexpr WgradFamily kWgradFamilies[] = {
    {"reg", 1, 4, WG_ANY, false, wgrad_reg_dispatch},                  // register-transposed loader
    {"glds", 5, 10, WG_16BIT, false, wgrad_glds_dispatch},             // LDS-DMA + transposed LDS reads
    {"nine_f32", 11, 16, WG_F32, true, wgrad9_f32_dispatch},           // nine taps, LDS-transposed tiles
    {"kmajor", 17, 20, WG_F32, false, wgrad_kmajor_dispatch},          // k-major MFMA operands, one tap
    {"nine_kmajor", 21, 24, WG_F32, true, wgrad9_kmajor_dispatch},     // nine taps, k-major operands
    {"nine_16", 25, 30, WG_16BIT, true, wgrad9t_h_dispatch},           // nine taps, transposed LDS reads
};

constexpr bool wgrad_families_sorted() {
    int prev = 0;
    for (const WgradFamily& f : kWgradFamilies) {
        if (f.first <= prev || f.last < f.first) return false;
        prev = f.last;
    }
    return true;
}
static_assert(wgrad_families_sorted(), "wgrad families must be sorted by first id and disjoint");

int wgrad_route(int dt, int tile, const WgradParams& p, hipStream_t st) {
    if (tile == 0) {  // by shape: the smallest tile that covers cout, wide tiles for wide layers
        tile = p.cout <= 16 ? 4 : p.cout <= 32 ? 3 : (p.cout >= 128 && p.cin >= 128) ? 2 : 1;
    }
    for (const WgradFamily& f : kWgradFamilies) {
        if (tile < f.first || tile > f.last) continue;
        if (!(f.dtypes & (dt == YXH_F32 ? WG_F32 : WG_16BIT))) {
            set_error("wgrad tiles %d-%d (%s) are built for %s only", f.first, f.last, f.name,
                      f.dtypes == WG_F32 ? "fp32" : "bf16/f16");
            return YXH_EUNSUPPORTED;
        }
        if (f.nine_tap && (p.kh != 3 || p.kw != 3 || p.pad != 1 || (p.stride != 1 && p.stride != 2))) {
            set_error("wgrad tiles %d-%d (%s, all nine taps per block) need a 3x3 pad-1 conv of stride 1 or 2",
                      f.first, f.last, f.name);
            return YXH_EUNSUPPORTED;
        }
        return f.fn(dt, tile, p, st);
    }
    set_error("wgrad tile %d", tile);
    return YXH_EINVAL;
}

}  // namespace

int conv_wgrad_launch(const yxh_wgrad_desc* d, hipStream_t st) {
    YXH_CHECK_ARG(d, "null descriptor");
    const int dt = d->dtype;
    YXH_CHECK_ARG(dt == YXH_F32 || dt == YXH_BF16 || dt == YXH_F16, "wgrad dtype %d", dt);
    const int epc = 16 / esz(dt);
    YXH_CHECK_ARG(d->batch > 0 && d->cin > 0 && d->cout > 0 && d->kh > 0 && d->kw > 0 && d->stride > 0,
                  "wgrad geometry");
    YXH_CHECK_ARG((d->in_h + 2 * d->pad - d->kh) / d->stride + 1 == d->out_h &&
                      (d->in_w + 2 * d->pad - d->kw) / d->stride + 1 == d->out_w,
                  "wgrad output size mismatch");
    YXH_CHECK_ARG(d->nsrc == 1 || d->nsrc == 2, "nsrc %d", d->nsrc);
    int chs = 0;
    for (int s = 0; s < d->nsrc; ++s) {
        const yxh_src& q = d->src[s];
        YXH_CHECK_ARG(q.ptr && a16(q.ptr) && q.channels % epc == 0 && q.cstride % epc == 0 && q.bstride % epc == 0,
                      "wgrad src%d alignment / channels", s);
        YXH_CHECK_ARG(q.upsample == 0 || q.upsample == 1, "wgrad src%d upsample %d", s, q.upsample);
        YXH_CHECK_ARG((q.h << q.upsample) == d->in_h && (q.w << q.upsample) == d->in_w, "wgrad src%d spatial", s);
        chs += q.channels;
    }
    YXH_CHECK_ARG(chs == d->cin, "wgrad source channels %d != cin %d", chs, d->cin);
    const yxh_src& g = d->dy;
    YXH_CHECK_ARG(g.ptr && a16(g.ptr) && g.channels % epc == 0 && g.channels >= d->cout && g.cstride % epc == 0 &&
                      g.bstride % epc == 0 && g.h == d->out_h && g.w == d->out_w && g.upsample == 0,
                  "wgrad dy view (channels %d must cover cout %d in %d-element chunks)", g.channels, d->cout, epc);
    YXH_CHECK_ARG(d->dw && d->cin_store > 0 && d->cin_store <= d->cin, "wgrad dw / cin_store");
    WgradParams p{};
    p.in_h = d->in_h; p.in_w = d->in_w; p.out_h = d->out_h; p.out_w = d->out_w;
    p.cin = d->cin; p.cout = d->cout; p.kh = d->kh; p.kw = d->kw; p.stride = d->stride; p.pad = d->pad;
    p.ohw = d->out_h * d->out_w;
    const long long M = (long long)d->batch * p.ohw;
    YXH_CHECK_ARG(M < (1LL << 31), "too many pixels");
    p.M = (int)M;
    p.B = d->batch;
    YXH_CHECK_ARG((long long)d->out_h * d->out_w * g.cstride < (1LL << 31) &&
                      (long long)d->src[0].h * d->src[0].w * d->src[0].cstride < (1LL << 31),
                  "wgrad: per-image offsets exceed 32 bits");
    p.nsrc = d->nsrc;
    p.src0_ch = d->src[0].channels;
    for (int s = 0; s < d->nsrc; ++s) {
        p.sptr[s] = d->src[s].ptr;
        p.scs[s] = d->src[s].cstride;
        p.sbs[s] = d->src[s].bstride;
        p.sw[s] = d->src[s].w;
        p.sup[s] = d->src[s].upsample;
    }
    p.dy = g.ptr;
    p.dycs = g.cstride;
    p.dybs = g.bstride;
    p.dw = d->dw;
    p.cin_store = d->cin_store;
    p.dych = g.channels;
    YXH_CHECK_ARG(!d->workspace || a16(d->workspace), "wgrad workspace alignment");
    p.ws = (float*)d->workspace;
    p.ws_elems = d->workspace ? d->workspace_bytes / 4 : 0;
    return wgrad_route(dt, d->tile, p, st);
}

}  // namespace yxh
