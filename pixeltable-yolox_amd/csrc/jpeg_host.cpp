// Host half of the JPEG decoder: header parsing, the Huffman (entropy) decode of one baseline
// scan into int16 coefficients, and the scalar restatement of the render stage.  Plain C++17 with
// no HIP headers: it is part of libyoloxhip.so and also builds on its own (tools/jpeg_check.cpp,
// with -DYXH_JPEG_STANDALONE for an error channel of its own).  No global state: every call
// keeps its tables on its stack, so calls from a thread pool need no lock.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include "jpeg_math.hpp"
#include "yoloxhip.h"

namespace yxh {
#ifdef YXH_JPEG_STANDALONE
static thread_local char g_jpeg_err[256] = "";
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_jpeg_err, sizeof(g_jpeg_err), fmt, ap);
    va_end(ap);
}
#else
void set_error(const char* fmt, ...);  // runtime.cpp
#endif
}  // namespace yxh

namespace {

using yxh::set_error;
namespace J = yxh::jpeg;

const uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                             41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                             30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct Huff {
    bool defined;
    uint16_t fast[512];    // 9-bit prefix -> (length << 8) | symbol, 0: longer than 9 bits or invalid
    int32_t maxcode[18];   // largest code of each length, -1 if none
    int32_t valoff[17];    // symbol index of a code = code + valoff[length]
    uint8_t vals[256];
};

struct Header {
    int height, width, ncomp, sampling;
    int comp_id[3], tq[3], td[3], ta[3];
    bool qdef[4];
    uint16_t quant[4][64];  // natural order
    Huff dc[4], ac[4];      // filled by decode only (want_tables)
    int restart;
    size_t scan;            // first byte of the entropy-coded data
};

int fail(int rc, const char* what) {
    set_error("jpeg: %s", what);
    return rc;
}

bool build_huff(Huff& h, const uint8_t counts[16], const uint8_t* vals, int nvals) {
    memset(h.fast, 0, sizeof(h.fast));
    memcpy(h.vals, vals, (size_t)nvals);
    int code = 0, k = 0;
    for (int len = 1; len <= 16; ++len) {
        const int n = counts[len - 1];
        h.valoff[len] = k - code;
        if (n) {
            if (code + n > (1 << len)) return false;  // over-subscribed code
            for (int i = 0; i < n; ++i, ++k, ++code)
                if (len <= 9)
                    for (int f = code << (9 - len), e = (code + 1) << (9 - len); f < e; ++f)
                        h.fast[f] = (uint16_t)((len << 8) | vals[k]);
            h.maxcode[len] = code - 1;
        } else {
            h.maxcode[len] = -1;
        }
        code <<= 1;
    }
    h.maxcode[17] = 0x7fffffff;
    h.defined = true;
    return true;
}

// Parse the markers from SOI up to and including SOS.  Huffman tables are built only when
// `want_tables` (the probe has no use for them, but checks them all the same for well-formedness).
int parse(const uint8_t* d, size_t len, Header& h, bool want_tables) {
    if (!d || len < 4 || d[0] != 0xFF || d[1] != 0xD8) return fail(YXH_EINVAL, "no SOI marker");
    h.ncomp = 0;
    h.restart = 0;
    for (int i = 0; i < 4; ++i) {
        h.qdef[i] = false;
        h.dc[i].defined = h.ac[i].defined = false;
    }
    bool jfif = false, adobe = false, sof = false;
    int transform = -1;
    size_t p = 2;
    for (;;) {
        if (p >= len || d[p] != 0xFF) return fail(YXH_EINVAL, "marker expected");
        while (p < len && d[p] == 0xFF) ++p;  // fill bytes
        if (p >= len) return fail(YXH_EINVAL, "truncated before the scan");
        const int m = d[p++];
        if (m == 0xD8 || m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;  // parameterless
        if (m == 0xD9) return fail(YXH_EINVAL, "EOI before any scan");
        if (m == 0x00) return fail(YXH_EINVAL, "stuffed byte outside a scan");
        if (p + 2 > len) return fail(YXH_EINVAL, "truncated segment length");
        const size_t n = ((size_t)d[p] << 8) | d[p + 1];
        if (n < 2 || p + n > len) return fail(YXH_EINVAL, "segment runs past the end");
        const uint8_t* s = d + p + 2;
        const size_t sl = n - 2;
        p += n;
        if (m == 0xC0) {
            if (sof) return fail(YXH_EINVAL, "second frame header");
            if (sl < 6) return fail(YXH_EINVAL, "short SOF0");
            sof = true;
            const int prec = s[0];
            h.height = (s[1] << 8) | s[2];
            h.width = (s[3] << 8) | s[4];
            const int nc = s[5];
            if (sl != (size_t)(6 + 3 * nc) || nc < 1) return fail(YXH_EINVAL, "bad SOF0 length");
            if (prec != 8) return fail(prec == 12 ? YXH_EUNSUPPORTED : YXH_EINVAL, "sample precision is not 8 bits");
            if (h.width == 0) return fail(YXH_EINVAL, "zero width");
            if (h.height == 0) return fail(YXH_EUNSUPPORTED, "height left to a DNL marker");
            if (nc != 1 && nc != 3)
                return fail(nc <= 4 ? YXH_EUNSUPPORTED : YXH_EINVAL, "neither 1 nor 3 components (CMYK / YCCK?)");
            int hs[3], vs[3];
            for (int c = 0; c < nc; ++c) {
                h.comp_id[c] = s[6 + 3 * c];
                hs[c] = s[7 + 3 * c] >> 4;
                vs[c] = s[7 + 3 * c] & 15;
                h.tq[c] = s[8 + 3 * c];
                if (hs[c] < 1 || hs[c] > 4 || vs[c] < 1 || vs[c] > 4 || h.tq[c] > 3)
                    return fail(YXH_EINVAL, "bad component parameters");
            }
            h.ncomp = nc;
            if (nc == 1) {
                h.sampling = YXH_JPEG_GRAY;  // a single component is never interleaved: factors are moot
            } else {
                if (hs[1] != 1 || vs[1] != 1 || hs[2] != 1 || vs[2] != 1)
                    return fail(YXH_EUNSUPPORTED, "chroma sampling is not 1x1");
                if (hs[0] == 1 && vs[0] == 1) h.sampling = YXH_JPEG_444;
                else if (hs[0] == 2 && vs[0] == 1) h.sampling = YXH_JPEG_422;
                else if (hs[0] == 2 && vs[0] == 2) h.sampling = YXH_JPEG_420;
                else return fail(YXH_EUNSUPPORTED, "luma sampling is not 1x1, 2x1 or 2x2 (4:4:0, 4:1:1, ...)");
            }
            if ((long long)h.height * h.width > J::kMaxPixels) return fail(YXH_EUNSUPPORTED, "more than 2^30 pixels");
        } else if (m == 0xC2 || m == 0xC6 || m == 0xCA || m == 0xCE) {
            return fail(YXH_EUNSUPPORTED, "progressive");
        } else if (m >= 0xC9 && m <= 0xCF && m != 0xCC) {
            return fail(YXH_EUNSUPPORTED, "arithmetic coding");
        } else if (m == 0xCC) {
            return fail(YXH_EUNSUPPORTED, "arithmetic conditioning table");
        } else if (m >= 0xC1 && m <= 0xC7 && m != 0xC4) {
            return fail(YXH_EUNSUPPORTED, "not a baseline (SOF0) frame");
        } else if (m == 0xC4) {
            size_t q = 0;
            while (q < sl) {
                if (q + 17 > sl) return fail(YXH_EINVAL, "short DHT");
                const int tc = s[q] >> 4, th = s[q] & 15;
                if (tc > 1 || th > 3) return fail(YXH_EINVAL, "bad DHT table id");
                int nv = 0;
                for (int i = 0; i < 16; ++i) nv += s[q + 1 + i];
                if (nv > 256 || q + 17 + (size_t)nv > sl) return fail(YXH_EINVAL, "bad DHT counts");
                Huff& t = tc ? h.ac[th] : h.dc[th];
                if (want_tables) {
                    if (!build_huff(t, s + q + 1, s + q + 17, nv)) return fail(YXH_EINVAL, "over-subscribed Huffman code");
                } else {
                    t.defined = true;
                }
                q += 17 + (size_t)nv;
            }
        } else if (m == 0xDB) {
            size_t q = 0;
            while (q < sl) {
                const int pq = s[q] >> 4, tq = s[q] & 15;
                if (tq > 3 || pq > 1) return fail(YXH_EINVAL, "bad DQT table id");
                if (pq) return fail(YXH_EUNSUPPORTED, "16-bit quantisation table");
                if (q + 65 > sl) return fail(YXH_EINVAL, "short DQT");
                for (int k = 0; k < 64; ++k) h.quant[tq][kZigzag[k]] = s[q + 1 + k];
                h.qdef[tq] = true;
                q += 65;
            }
        } else if (m == 0xDD) {
            if (sl != 2) return fail(YXH_EINVAL, "bad DRI length");
            h.restart = (s[0] << 8) | s[1];
        } else if (m == 0xDC) {
            return fail(YXH_EUNSUPPORTED, "DNL marker");
        } else if (m == 0xE0) {
            if (sl >= 14 && memcmp(s, "JFIF\0", 5) == 0) jfif = true;
        } else if (m == 0xEE) {
            if (sl >= 12 && memcmp(s, "Adobe", 5) == 0) {
                adobe = true;
                transform = s[11];
            }
        } else if (m == 0xDA) {
            if (!sof) return fail(YXH_EINVAL, "scan before the frame header");
            if (sl < 1) return fail(YXH_EINVAL, "short SOS");
            const int ns = s[0];
            if (ns < 1 || ns > 4 || sl != (size_t)(4 + 2 * ns)) return fail(YXH_EINVAL, "bad SOS length");
            if (ns != h.ncomp) return fail(ns < h.ncomp ? YXH_EUNSUPPORTED : YXH_EINVAL, "more than one scan");
            for (int c = 0; c < ns; ++c) {
                if (s[1 + 2 * c] != h.comp_id[c]) return fail(YXH_EUNSUPPORTED, "scan components out of frame order");
                h.td[c] = s[2 + 2 * c] >> 4;
                h.ta[c] = s[2 + 2 * c] & 15;
                if (h.td[c] > 3 || h.ta[c] > 3) return fail(YXH_EINVAL, "bad scan table id");
                if (!h.dc[h.td[c]].defined || !h.ac[h.ta[c]].defined) return fail(YXH_EINVAL, "scan uses an undefined Huffman table");
                if (!h.qdef[h.tq[c]]) return fail(YXH_EINVAL, "component uses an undefined quantisation table");
            }
            if (s[1 + 2 * ns] != 0 || s[2 + 2 * ns] != 63 || s[3 + 2 * ns] != 0)
                return fail(YXH_EINVAL, "baseline scan with a spectral selection or successive approximation");
            if (h.ncomp == 3) {  // libjpeg's colour space guess (jdapimin.c default_decompress_parms)
                if (!jfif && adobe && transform != 1)
                    return fail(YXH_EUNSUPPORTED, "Adobe marker without a YCbCr transform");
                if (!jfif && !adobe && h.comp_id[0] == 'R' && h.comp_id[1] == 'G' && h.comp_id[2] == 'B')
                    return fail(YXH_EUNSUPPORTED, "components are labelled R, G, B");
            }
            h.scan = p;
            return YXH_OK;
        }
        // every other segment (APPn, COM, ...) is skipped
    }
}

// MSB-first bit reader over the entropy-coded segment: FF 00 is a data byte FF, any other marker
// (or the end of the input) ends the data; past it the reader supplies zero bits and counts them,
// and the caller treats having consumed any as an error.
struct Bits {
    const uint8_t* d;
    size_t pos, len;
    uint64_t buf;  // the next bits at the top
    int n;         // bits in buf
    int fake;      // how many of them (at the tail) are made up

    void fill() {
        while (n <= 56) {
            unsigned b = 0;
            bool real = false;
            if (!fake && pos < len) {
                if (d[pos] != 0xFF) {
                    b = d[pos++];
                    real = true;
                } else if (pos + 1 < len && d[pos + 1] == 0x00) {
                    b = 0xFF;
                    pos += 2;
                    real = true;
                }
            }
            if (!real) fake += 8;
            buf |= (uint64_t)b << (56 - n);
            n += 8;
        }
    }
    // one Huffman code (<= 16 bits) and its value bits (<= 15) never need more than 31 bits
    void need31() {
        if (n < 32) fill();
    }
    unsigned peek(int k) { return (unsigned)(buf >> (64 - k)); }  // 1 <= k <= 32, of bits need31() assured
    void skip(int k) {
        buf <<= k;
        n -= k;
    }
    bool overrun() const { return n < fake; }
};

inline int decode_symbol(Bits& b, const Huff& h) {
    const unsigned f = h.fast[b.peek(9)];
    if (f) {
        b.skip((int)(f >> 8));
        return (int)(f & 255);
    }
    const int code16 = (int)b.peek(16);
    for (int len = 10; len <= 16; ++len) {
        const int code = code16 >> (16 - len);
        if (code <= h.maxcode[len]) {
            b.skip(len);
            return h.vals[(code + h.valoff[len]) & 255];
        }
    }
    return -1;
}

inline int receive_extend(Bits& b, int s) {
    const int v = (int)b.peek(s);
    b.skip(s);
    return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

int decode_block(Bits& b, const Huff& dc, const Huff& ac, int& pred, int16_t* out) {
    b.need31();
    int s = decode_symbol(b, dc);
    if (s < 0 || s > 11) return fail(YXH_EINVAL, "bad DC code");
    if (s) pred += receive_extend(b, s);
    if (pred < -32768 || pred > 32767) return fail(YXH_EINVAL, "DC value out of range");
    out[0] = (int16_t)pred;
    for (int k = 1; k < 64;) {
        b.need31();
        const int rs = decode_symbol(b, ac);
        if (rs < 0) return fail(YXH_EINVAL, "bad AC code");
        const int r = rs >> 4;
        s = rs & 15;
        if (s == 0) {
            if (r != 15) break;
            k += 16;
            continue;
        }
        k += r;
        if (k > 63) return fail(YXH_EINVAL, "AC run past the block");
        out[kZigzag[k]] = (int16_t)receive_extend(b, s);
        ++k;
    }
    return YXH_OK;
}

void fill_image(const Header& h, const J::Geom& g, yxh_jpeg_image* im) {
    memset(im, 0, sizeof(*im));
    im->height = h.height;
    im->width = h.width;
    im->components = h.ncomp;
    im->sampling = h.sampling;
    for (int c = 0; c < h.ncomp; ++c) {
        im->blocks_w[c] = g.bw[c];
        im->blocks_h[c] = g.bh[c];
        im->comp_block0[c] = (int32_t)g.blk0[c];
        memcpy(im->quant[c], h.quant[h.tq[c]], sizeof(im->quant[c]));
    }
}

}  // namespace

extern "C" {

int yxh_jpeg_probe(const uint8_t* data, size_t len, yxh_jpeg_info* info) {
    if (!data || !info) return fail(YXH_EINVAL, "null pointer");
    Header h;
    const int rc = parse(data, len, h, false);
    if (rc != YXH_OK) return rc;
    J::Geom g;
    if (!J::geom(h.height, h.width, h.ncomp, h.sampling, g)) return fail(YXH_EINVAL, "impossible size");
    info->height = h.height;
    info->width = h.width;
    info->components = h.ncomp;
    info->sampling = h.sampling;
    info->coef_bytes = g.blk0[3] * 128;
    return YXH_OK;
}

int yxh_jpeg_decode(const uint8_t* data, size_t len, int16_t* coef, size_t coef_bytes, yxh_jpeg_image* image) {
    if (!data || !coef || !image) return fail(YXH_EINVAL, "null pointer");
    Header h;
    int rc = parse(data, len, h, true);
    if (rc != YXH_OK) return rc;
    J::Geom g;
    if (!J::geom(h.height, h.width, h.ncomp, h.sampling, g)) return fail(YXH_EINVAL, "impossible size");
    const size_t need = (size_t)g.blk0[3] * 128;
    if (coef_bytes < need) return fail(YXH_EINVAL, "coefficient buffer too small");
    memset(coef, 0, need);
    const int hmax = g.ncomp == 1 ? 1 : g.bw[0] / g.bw[1], vmax = g.ncomp == 1 ? 1 : g.bh[0] / g.bh[1];
    const int mx = g.bw[0] / hmax, my = g.bh[0] / vmax;
    Bits b = {data, h.scan, len, 0, 0, 0};
    int pred[3] = {0, 0, 0};
    int left = h.restart, next_rst = 0;
    for (int y = 0; y < my; ++y) {
        for (int x = 0; x < mx; ++x) {
            if (h.restart && left == 0) {
                // byte-align, then exactly the expected RSTn (fill bytes allowed in front of it)
                if (b.overrun() || b.n - b.fake >= 8) return fail(YXH_EINVAL, "data where a restart marker belongs");
                size_t p = b.pos;
                if (p >= len || data[p] != 0xFF) return fail(YXH_EINVAL, "restart marker missing");
                while (p < len && data[p] == 0xFF) ++p;
                if (p >= len || data[p] != 0xD0 + next_rst) return fail(YXH_EINVAL, "wrong restart marker");
                b.pos = p + 1;
                b.buf = 0;
                b.n = b.fake = 0;
                pred[0] = pred[1] = pred[2] = 0;
                next_rst = (next_rst + 1) & 7;
                left = h.restart;
            }
            for (int c = 0; c < g.ncomp; ++c) {
                const int ch = c == 0 ? hmax : 1, cv = c == 0 ? vmax : 1;
                for (int v = 0; v < cv; ++v)
                    for (int u = 0; u < ch; ++u) {
                        const long long blk = g.blk0[c] + (long long)(y * cv + v) * g.bw[c] + (x * ch + u);
                        rc = decode_block(b, h.dc[h.td[c]], h.ac[h.ta[c]], pred[c], coef + blk * 64);
                        if (rc != YXH_OK) return rc;
                    }
            }
            if (b.overrun()) return fail(YXH_EINVAL, "entropy-coded data ends early");
            --left;
        }
    }
    fill_image(h, g, image);
    return YXH_OK;
}

size_t yxh_jpeg_workspace_bytes(int32_t height, int32_t width, int32_t sampling) {
    J::Geom g;
    if (!J::geom(height, width, sampling == YXH_JPEG_GRAY ? 1 : 3, sampling, g)) return 0;
    return (size_t)((g.plane[3] + 15) & ~15ll);
}

int yxh_jpeg_render_host(const int16_t* coef, const yxh_jpeg_image* images, int32_t batch, uint8_t* workspace,
                         uint8_t* dst) {
    if (!coef || !images || !workspace || !dst) return fail(YXH_EINVAL, "render: null pointer");
    if (batch < 1) return fail(YXH_EINVAL, "render: empty batch");
    for (int i = 0; i < batch; ++i) {
        const yxh_jpeg_image& im = images[i];
        J::Geom g;
        if (!J::offsets_ok(im) || !J::geom(im.height, im.width, im.components, im.sampling, g)) continue;
        const int16_t* cf = coef + im.coef_offset / 2;
        uint8_t* ws = workspace + im.ws_offset;
        for (int c = 0; c < g.ncomp; ++c) {
            const long long stride = (long long)g.bw[c] * 8;
            for (int by = 0; by < g.bh[c]; ++by)
                for (int bx = 0; bx < g.bw[c]; ++bx)
                    J::idct_block(cf + (g.blk0[c] + (long long)by * g.bw[c] + bx) * 64, im.quant[c],
                                  ws + g.plane[c] + (long long)by * 8 * stride + bx * 8, stride);
        }
        uint8_t* o = dst + im.dst_offset;
        for (int y = 0; y < im.height; ++y)
            for (int x = 0; x < im.width; ++x, o += 3) {
                int rgb[3];
                J::pixel_rgb(ws, g, im.sampling, x, y, rgb);
                o[0] = (uint8_t)rgb[0];
                o[1] = (uint8_t)rgb[1];
                o[2] = (uint8_t)rgb[2];
            }
    }
    return YXH_OK;
}

size_t yxh_sizeof_jpeg_info(void) { return sizeof(yxh_jpeg_info); }
size_t yxh_sizeof_jpeg_image(void) { return sizeof(yxh_jpeg_image); }

#ifdef YXH_JPEG_STANDALONE
const char* yxh_last_error(void) { return yxh::g_jpeg_err; }
#endif

}  // extern "C"
