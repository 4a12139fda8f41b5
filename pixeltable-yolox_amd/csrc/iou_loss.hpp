// IouLoss for one (pred, target) box pair -- reference yolox/models/losses.py:13-51.
// The one statement of the formula in the tree: the SimOTA loss kernels (simota.hip)
// and the standalone IouLoss kernels (iou_loss.hip) both call these functions.
//
// Boxes are (cx, cy, w, h).  Every expression keeps the reference's fp32 operation
// order (tl / br, area_p, area_g, en, area_i, area_u, iou, then the type's tail), so the
// forward value is the reference's to the bit where torch's ops round like these.
// The backward is torch's autograd rule by rule:
//   torch.max / torch.min of two tensors : full gradient to the selected side, half to
//                                          each on a tie (tie_w), for tl / br and c_tl / c_br
//   giou.clamp(-1, 1)                    : passes on the closed interval
//   area_c.clamp(1e-16)                  : passes for area_c >= 1e-16, blocked below
//   a / b                                : grad / b  and  -grad * ((a / b) / b)
//   en                                   : a comparison, carries no gradient
#pragma once
#pragma clang fp contract(off)  // round like torch's separate ops

#include "yxh_common.hpp"

namespace yxh {

__device__ __forceinline__ float tie_w(float a, float b, bool want_greater) {
    // torch.maximum / minimum backward: full gradient to the selected input, half on ties
    if (a == b) return 0.5f;
    return (want_greater ? a > b : a < b) ? 1.0f : 0.0f;
}

// loss of one pair; TYPE is YXH_IOU_LOSS_IOU or YXH_IOU_LOSS_GIOU
template <int TYPE>
__device__ __forceinline__ float iou_loss_pair(const float* p, const float* t) {
    const float atx = p[0] - p[2] / 2, btx = t[0] - t[2] / 2, aty = p[1] - p[3] / 2, bty = t[1] - t[3] / 2;
    const float abx = p[0] + p[2] / 2, bbx = t[0] + t[2] / 2, aby = p[1] + p[3] / 2, bby = t[1] + t[3] / 2;
    const float tlx = fmaxf(atx, btx), tly = fmaxf(aty, bty);
    const float brx = fminf(abx, bbx), bry = fminf(aby, bby);
    const float area_p = p[2] * p[3], area_g = t[2] * t[3];
    const float en = (tlx < brx && tly < bry) ? 1.0f : 0.0f;
    const float area_i = ((brx - tlx) * (bry - tly)) * en;
    const float area_u = (area_p + area_g) - area_i;
    const float io = area_i / (area_u + 1e-16f);
    if (TYPE == YXH_IOU_LOSS_IOU) return 1.0f - io * io;
    const float ctlx = fminf(atx, btx), ctly = fminf(aty, bty);
    const float cbrx = fmaxf(abx, bbx), cbry = fmaxf(aby, bby);
    const float area_c = (cbrx - ctlx) * (cbry - ctly);
    const float giou = io - (area_c - area_u) / fmaxf(area_c, 1e-16f);
    return 1.0f - fminf(fmaxf(giou, -1.0f), 1.0f);
}

// go = d L / d loss of this pair.  gp[4] = d L / d pred; gt[4] = d L / d target when WANT_T.
template <int TYPE, bool WANT_T>
__device__ __forceinline__ void iou_loss_pair_bwd(const float* p, const float* t, float go, float* gp, float* gt) {
    const float px = p[0], py = p[1], pw = p[2], ph = p[3];
    const float atx = px - pw / 2, btx = t[0] - t[2] / 2, aty = py - ph / 2, bty = t[1] - t[3] / 2;
    const float abx = px + pw / 2, bbx = t[0] + t[2] / 2, aby = py + ph / 2, bby = t[1] + t[3] / 2;
    const float tlx = fmaxf(atx, btx), tly = fmaxf(aty, bty), brx = fminf(abx, bbx), bry = fminf(aby, bby);
    const float en = (tlx < brx && tly < bry) ? 1.0f : 0.0f;
    const float dxx = brx - tlx, dyy = bry - tly;
    const float ai = (dxx * dyy) * en;
    const float ap = pw * ph, ag = t[2] * t[3];
    const float au = (ap + ag) - ai;
    const float u = au + 1e-16f;
    const float io = ai / u;
    float gi;                                  // d L / d iou
    float gau = 0.0f, gcw = 0.0f, gch = 0.0f;  // giou only: d L / d area_u (its own use), d L / d (c_br - c_tl)
    if (TYPE == YXH_IOU_LOSS_IOU) {
        gi = go * (-2.0f * io);
    } else {
        const float ctlx = fminf(atx, btx), ctly = fminf(aty, bty), cbrx = fmaxf(abx, bbx), cbry = fmaxf(aby, bby);
        const float cw = cbrx - ctlx, ch = cbry - ctly;
        const float ac = cw * ch;
        const float q = ac - au;
        const float m = fmaxf(ac, 1e-16f);
        const float r = q / m;
        const float giou = io - r;
        gi = (giou >= -1.0f && giou <= 1.0f) ? -go : 0.0f;
        const float gr = -gi;
        const float gq = gr / m;
        const float gm = -gr * (r / m);
        const float gac = ac >= 1e-16f ? gq + gm : gq;
        gau = -gq;
        gcw = gac * ch;
        gch = gac * cw;
    }
    const float gu = -gi * ai / (u * u);
    float gai = gi / u - gu;
    float gap = gu;
    if (TYPE != YXH_IOU_LOSS_IOU) {
        gai = gai - gau;
        gap = gap + gau;
    }
    const float gdx = gai * en * dyy, gdy = gai * en * dxx;
    const float gtlx = -gdx * tie_w(atx, btx, true), gbrx = gdx * tie_w(abx, bbx, false);
    const float gtly = -gdy * tie_w(aty, bty, true), gbry = gdy * tie_w(aby, bby, false);
    float gpx = gtlx + gbrx, gpy = gtly + gbry;
    float gpw = 0.5f * (gbrx - gtlx) + gap * ph;
    float gph = 0.5f * (gbry - gtly) + gap * pw;
    if (TYPE != YXH_IOU_LOSS_IOU) {
        const float cl = -gcw * tie_w(atx, btx, false), cr = gcw * tie_w(abx, bbx, true);
        const float ct = -gch * tie_w(aty, bty, false), cb = gch * tie_w(aby, bby, true);
        gpx = gpx + (cl + cr);
        gpy = gpy + (ct + cb);
        gpw = gpw + 0.5f * (cr - cl);
        gph = gph + 0.5f * (cb - ct);
    }
    gp[0] = gpx;
    gp[1] = gpy;
    gp[2] = gpw;
    gp[3] = gph;
    if (WANT_T) {
        const float ttlx = -gdx * tie_w(btx, atx, true), tbrx = gdx * tie_w(bbx, abx, false);
        const float ttly = -gdy * tie_w(bty, aty, true), tbry = gdy * tie_w(bby, aby, false);
        float gx = ttlx + tbrx, gy = ttly + tbry;
        float gw = 0.5f * (tbrx - ttlx) + gap * t[3];
        float gh = 0.5f * (tbry - ttly) + gap * t[2];
        if (TYPE != YXH_IOU_LOSS_IOU) {
            const float cl = -gcw * tie_w(btx, atx, false), cr = gcw * tie_w(bbx, abx, true);
            const float ct = -gch * tie_w(bty, aty, false), cb = gch * tie_w(bby, aby, true);
            gx = gx + (cl + cr);
            gy = gy + (ct + cb);
            gw = gw + 0.5f * (cr - cl);
            gh = gh + 0.5f * (cb - ct);
        }
        gt[0] = gx;
        gt[1] = gy;
        gt[2] = gw;
        gt[3] = gh;
    }
}

}  // namespace yxh
