// reloc_orb_plan.h -- the geometry of one ORB frame size, worked out on the host: levels, quotas, tile bases, resize tables,
// the rectangles of the fused pyramid's tiles and its LDS layout (orb_plan), and the sizes of the blocks that hold them
// (orb_caps).  Plain C++ without HIP: the library uploads a plan (orb_prepare, reloc_orb.hip), tests/host/orb_plan_check.cpp
// sweeps it on the CPU.  The level, table and tile types are the ones the kernels read; their layout is part of the device code.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/reloc.h"
#include "../../include/reloc_spec.h"

constexpr int NLEV = RELOC_ORB_NLEVELS;

// tiles of the ORB kernels
#ifndef PYR_TW
#define PYR_TW 64
#define PYR_TH 32
#endif
constexpr int PT_W = PYR_TW, PT_H = PYR_TH;     // k_pyramid: level-0 footprint of a tile
constexpr int FT = 32;                          // FAST + NMS: FT x FT tiles over (stride x h)
constexpr int BT_W = 64, BT_H = 16;             // blur: tiles over (w x h)
constexpr int HARRIS_CHUNK = 1024;              // bytes of the NMS map per k_harris block (4 per thread)
constexpr int PYR_LDS_MAX = 64 * 1024;          // LDS a workgroup of k_pyramid may ask for

struct OrbLevel {
    int w, h;          // level size
    int stride;        // row stride in bytes (multiple of 64)
    int64_t off;       // byte offset of the level inside a pyramid buffer
    float scale;
    int quota;
};

// cv2.ORB_create's runtime parameters (include/reloc_spec.h "ORB PARAMS"); the defaults are the detector of a context that
// never set any.  Levels >= nlevels of a plan are empty.
struct OrbParams {
    int nlevels = RELOC_ORB_NLEVELS;
    double scale = RELOC_ORB_SCALE_FACTOR;
    int fast_thr = RELOC_FAST_THRESHOLD;
    int score = RELOC_ORB_HARRIS_SCORE;
    bool same(const OrbParams &o) const { return nlevels == o.nlevels && scale == o.scale && fast_thr == o.fast_thr && score == o.score; }
    // NULL, or the range that a value leaves
    const char *check() const
    {
        if (nlevels < RELOC_ORB_NLEVELS_MIN || nlevels > RELOC_ORB_NLEVELS) return "nlevels outside 1..8";
        if (!(scale >= RELOC_ORB_SCALE_MIN && scale <= RELOC_ORB_SCALE_MAX)) return "scaleFactor not finite or outside 1.01..2.0";
        if (fast_thr < RELOC_FAST_THRESHOLD_MIN || fast_thr > RELOC_FAST_THRESHOLD_MAX) return "fastThreshold outside 1..254";
        if (score != RELOC_ORB_HARRIS_SCORE && score != RELOC_ORB_FAST_SCORE) return "scoreType outside 0..1 (HARRIS_SCORE, FAST_SCORE)";
        return nullptr;
    }
};

struct OrbTable {
    OrbLevel lev[NLEV];
    int fast_tile_base[NLEV + 1];   // 32x32 tiles over (stride x h)
    int blur_tile_base[NLEV + 1];   // 64x16 tiles over (w x h)
    int flat_base[NLEV + 1];        // HARRIS_CHUNK-byte chunks over stride*h
    int rz_off[NLEV][4];            // offsets into the resize table: xofs, xcoef, yofs, ycoef
    int nlevels;                    // levels in use; the ones behind them are empty
    int fast_thr;                   // FAST threshold, read by the kernels that are not built for the default
    int score;                      // RELOC_ORB_HARRIS_SCORE | RELOC_ORB_FAST_SCORE
    int pad;
};
static_assert(sizeof(OrbLevel) == 32 && sizeof(OrbTable) == 512, "OrbTable is read by every ORB kernel");

struct PyrTile {
    uint16_t o[NLEV][4];    // stored rectangle x0, x1, y0, y1 (x0 multiple of 4; x1 may reach into the row padding)
    uint16_t n[NLEV][4];    // computed rectangle (x0 multiple of 4, x1 <= level width)
};
static_assert(sizeof(PyrTile) == 128, "PyrTile is read as 8 dwordx4");

struct PyrLds { int lev[NLEV]; int tabs; };    // byte offsets of the level buffers and of the table slices in LDS

// What a context of capacity max_w x max_h reserves for the geometry of any frame within it (orb_alloc)
struct OrbCaps {
    int64_t pyr_bytes;      // one pyramid buffer: every level's rows, each level rounded up to 256 bytes
    int64_t rz_entries;     // int32 entries of the resize tables
    int64_t tiles;          // PyrTile entries
};

static inline OrbCaps orb_caps(int max_w, int max_h, const OrbParams &prm = OrbParams{})
{
    OrbCaps c;
    // a level is at most 1 + dim / scale wide and high (lrintf), its stride the width rounded up to 64
    c.pyr_bytes = 0;
    for (int l = 0; l < prm.nlevels; ++l) {
        const double s = pow(prm.scale, (double)l);
        const int64_t w = (int64_t)(max_w / s) + 2, h = (int64_t)(max_h / s) + 2;
        c.pyr_bytes += ((w + 63) / 64 * 64) * h + 256;
    }
    // per level and axis one offset and one coefficient per pixel of the level, no level larger than the frame
    c.rz_entries = (int64_t)NLEV * 2 * 2 * (max_w > max_h ? max_w : max_h);
    c.tiles = (int64_t)((max_w + PT_W - 1) / PT_W) * ((max_h + PT_H - 1) / PT_H);
    return c;
}

struct OrbPlan {
    int rc = RELOC_OK;              // RELOC_E_CAPACITY: err says what does not fit, nothing else is valid
    const char *err = nullptr;
    OrbTable tab;
    std::vector<int32_t> rz;        // resize tables, addressed by tab.rz_off
    std::vector<PyrTile> tiles;     // one per workgroup of k_pyramid
    PyrLds lds;
    int lds_bytes = 0;              // dynamic LDS of k_pyramid: the level buffers, then the table slices
};

// INTER_LINEAR_EXACT taps of one axis: source offset and 8-bit coefficient of every destination pixel
static inline void orb_resize_axis(int src_n, int dst_n, int32_t *ofs, int32_t *coef)
{
    const double scale = (double)src_n / (double)dst_n;
    for (int d = 0; d < dst_n; ++d) {
        double f = ((double)d + 0.5) * scale - 0.5;
        int s = (int)floor(f);
        double a = f - (double)s;
        if (s < 0) { s = 0; a = 0.0; }
        if (s >= src_n - 1) { s = src_n - 1; a = 0.0; }
        ofs[d] = s;
        coef[d] = (int32_t)lrint(a * (double)(1 << RELOC_RESIZE_COEF_BITS));
    }
}

// The plan of a w x h frame with nfeatures keypoints for blocks of the sizes in caps.
// Levels l >= prm.nlevels are empty (w = h = stride = 0, quota 0): they own no tile, no table entry and no byte of a tile's
// rectangles, and the kernels' NLEV-long loops fall through them.  So is a level whose width or height rounds to 0 (a frame
// below scale^l / 2: never with the default parameters from 64 x 64 on), whatever its quota.
static inline OrbPlan orb_plan(int w, int h, int nfeatures, const OrbCaps &caps, const OrbParams &prm = OrbParams{})
{
    OrbPlan p;
    OrbTable &tab = p.tab;
    memset(&tab, 0, sizeof(tab));
    memset(&p.lds, 0, sizeof(p.lds));
    auto refuse = [&p](const char *what) { p.rc = RELOC_E_CAPACITY; p.err = what; };
    if (prm.check()) { p.rc = RELOC_E_ARG; p.err = prm.check(); return p; }
    if (w > 0xFFFF || h > 0xFFFF) { refuse("frame exceeds the 16-bit rectangles of the pyramid tiles"); return p; }
    const int nlev = prm.nlevels;
    tab.nlevels = nlev; tab.fast_thr = prm.fast_thr; tab.score = prm.score;
    int64_t off = 0;
    for (int l = 0; l < NLEV; ++l) {
        const float s = (float)pow(prm.scale, (double)l);
        OrbLevel &L = tab.lev[l];
        L.scale = s;
        L.off = off;
        if (l >= nlev) continue;
        L.w = (int)lrintf((float)w / s);
        L.h = (int)lrintf((float)h / s);
        if (L.w < 1 || L.h < 1) L.w = L.h = 0;      // rounded away (scale^l beyond twice the frame): empty like the levels behind nlevels
        L.stride = (L.w + 63) / 64 * 64;
        off += ((int64_t)L.stride * L.h + 255) / 256 * 256;
    }
    if (off > caps.pyr_bytes) { refuse("pyramid arena too small"); return p; }
    {
        const float factor = (float)(1.0 / prm.scale);
        float nper = (float)(nfeatures * (1 - factor) / (1 - (float)pow((double)factor, (double)nlev)));
        int sum = 0;
        for (int l = 0; l < nlev - 1; ++l) {
            tab.lev[l].quota = (int)lrintf(nper);
            sum += tab.lev[l].quota;
            nper *= factor;
        }
        tab.lev[nlev - 1].quota = nfeatures - sum > 0 ? nfeatures - sum : 0;
    }
    for (int l = 0; l < NLEV; ++l) {
        const OrbLevel &L = tab.lev[l];
        tab.fast_tile_base[l + 1] = tab.fast_tile_base[l] + (L.stride / FT) * ((L.h + FT - 1) / FT);
        tab.blur_tile_base[l + 1] = tab.blur_tile_base[l] + ((L.w + BT_W - 1) / BT_W) * ((L.h + BT_H - 1) / BT_H);
        tab.flat_base[l + 1] = tab.flat_base[l] + (int)(((int64_t)L.stride * L.h + HARRIS_CHUNK - 1) / HARRIS_CHUNK);
    }
    // resize tables
    int64_t pos = 0;
    for (int l = 1; l < NLEV; ++l) {
        const OrbLevel &D = tab.lev[l];
        tab.rz_off[l][0] = (int)pos; tab.rz_off[l][1] = (int)pos + D.w;
        pos += 2 * D.w;
        tab.rz_off[l][2] = (int)pos; tab.rz_off[l][3] = (int)pos + D.h;
        pos += 2 * D.h;
    }
    if (pos > caps.rz_entries) { refuse("resize tables exceed their block"); return p; }
    p.rz.resize((size_t)pos);
    int32_t *host = p.rz.data();
    for (int l = 1; l < nlev; ++l) {
        const OrbLevel &S = tab.lev[l - 1], &D = tab.lev[l];
        if (D.w < 1) continue;
        orb_resize_axis(S.w, D.w, host + tab.rz_off[l][0], host + tab.rz_off[l][1]);
        orb_resize_axis(S.h, D.h, host + tab.rz_off[l][2], host + tab.rz_off[l][3]);
    }
    // fused-pyramid tiles: every tile owns a rectangle of every level (proportional split, x on 4-pixel
    // boundaries, the last column of tiles takes the row padding of levels >= 1, which is stored as 0)
    // and computes what the levels above need from it (k_pyramid).
    const int ntx = (w + PT_W - 1) / PT_W, nty = (h + PT_H - 1) / PT_H;
    if ((int64_t)ntx * nty > caps.tiles) { refuse("pyramid tiles exceed their block"); return p; }
    p.tiles.resize((size_t)ntx * nty);
    memset(p.tiles.data(), 0, sizeof(PyrTile) * p.tiles.size());
    int lds_lev[NLEV] = {}, lds_t = 0;
    for (int t = 0; t < ntx * nty; ++t) {
        const int tx = t % ntx, ty = t / ntx;
        PyrTile &T = p.tiles[t];
        int nx0 = 0, nx1 = 0, ny0 = 0, ny1 = 0;    // needed rectangle of the level above (empty)
        int tsum = 0;
        for (int l = NLEV - 1; l >= 0; --l) {
            const OrbLevel &L = tab.lev[l];
            const int quads = (l == 0 ? (L.w + 3) / 4 : L.stride / 4);
            const int ox0 = 4 * (int)((int64_t)tx * quads / ntx), ox1 = 4 * (int)((int64_t)(tx + 1) * quads / ntx);
            const int oy0 = (int)((int64_t)ty * L.h / nty), oy1 = (int)((int64_t)(ty + 1) * L.h / nty);
            T.o[l][0] = (uint16_t)ox0; T.o[l][1] = (uint16_t)ox1; T.o[l][2] = (uint16_t)oy0; T.o[l][3] = (uint16_t)oy1;
            // computed rectangle = own pixels (inside the image) united with the taps of the level above
            int cx0 = ox0, cx1 = ox1 < L.w ? ox1 : L.w, cy0 = oy0, cy1 = oy1;
            const bool stores = ox0 < ox1 && oy0 < oy1;                     // may be row padding only
            const bool own = cx0 < cx1 && cy0 < cy1, need = nx0 < nx1 && ny0 < ny1;
            if (need) {
                const int32_t *xo = host + tab.rz_off[l + 1][0], *yo = host + tab.rz_off[l + 1][2];
                int sx0 = xo[nx0], sx1 = xo[nx1 - 1] + 2, sy0 = yo[ny0], sy1 = yo[ny1 - 1] + 2;
                if (sx1 > L.w) sx1 = L.w;
                if (sy1 > L.h) sy1 = L.h;
                if (own) {
                    cx0 = cx0 < sx0 ? cx0 : sx0; cx1 = cx1 > sx1 ? cx1 : sx1;
                    cy0 = cy0 < sy0 ? cy0 : sy0; cy1 = cy1 > sy1 ? cy1 : sy1;
                } else {
                    cx0 = sx0; cx1 = sx1; cy0 = sy0; cy1 = sy1;
                }
            } else if (!own) {
                cx0 = cx1 = cy0 = cy1 = 0;
            }
            cx0 &= ~3;
            T.n[l][0] = (uint16_t)cx0; T.n[l][1] = (uint16_t)cx1; T.n[l][2] = (uint16_t)cy0; T.n[l][3] = (uint16_t)cy1;
            if (!stores) T.o[l][0] = T.o[l][1] = T.o[l][2] = T.o[l][3] = 0;
            nx0 = cx0; nx1 = cx1; ny0 = cy0; ny1 = cy1;
            const int bytes = ((cx1 - cx0 + 3) / 4 * 4) * (cy1 - cy0);
            lds_lev[l] = bytes > lds_lev[l] ? bytes : lds_lev[l];
            if (l >= 1) tsum += (cx1 - cx0) + (cy1 - cy0);
        }
        lds_t = tsum > lds_t ? tsum : lds_t;
    }
    int o = 0;
    for (int l = 0; l < NLEV; ++l) { p.lds.lev[l] = o; o += (lds_lev[l] + 15) / 16 * 16; }
    p.lds.tabs = o;
    p.lds_bytes = o + 4 * lds_t;
    if (p.lds_bytes > PYR_LDS_MAX) refuse("pyramid tile exceeds LDS");
    return p;
}
