// orb_plan_check.cpp -- sweeps orb_plan (csrc/reloc_orb_plan.h) on the CPU: what k_pyramid and the other ORB kernels assume of
// the tables and tiles of a frame size, checked for every size of the sweep.  Stand-alone: includes the plan header alone.
//   orb_plan_check               the sweep; prints one summary line, exit status 1 and the first failures otherwise
//   orb_plan_check levels W H    prints "w h" of the NLEV levels of a W x H frame
// tests/test_orb_plan_host.py builds and runs it.
#include <stdio.h>
#include <stdlib.h>

#include "../../nclt-slam-project_amd/csrc/reloc_orb_plan.h"

static int g_w, g_h, g_failures;
static int g_max_lds, g_max_w, g_max_h;      // the largest LDS request of the sweep

#define CHECK(cond, ...)                                                   \
    do {                                                                   \
        if (!(cond)) {                                                     \
            printf("FAIL %dx%d: %s: ", g_w, g_h, #cond);                   \
            printf(__VA_ARGS__);                                           \
            printf("\n");                                                  \
            if (++g_failures >= 20) exit(1);                               \
        }                                                                  \
    } while (0)

struct Span { int a = 0, b = 0; bool set = false; };

// The spans of a grid's columns (or rows) partition [0, end): in index order, each begins where the one before ended.
static bool partitions(const std::vector<Span> &s, int end)
{
    int at = 0;
    for (const Span &x : s) {
        if (!x.set) continue;
        if (x.a != at || x.b <= x.a) return false;
        at = x.b;
    }
    return at == end;
}

static int pitch_of(const uint16_t r[4]) { return ((r[1] - r[0] + 3) >> 2) << 2; }
static bool empty_rect(const uint16_t r[4]) { return r[0] >= r[1] || r[2] >= r[3]; }

static void check_size(int w, int h, int nfeatures)
{
    g_w = w; g_h = h;
    const OrbCaps caps = orb_caps(w, h);                    // the capacity is the frame itself
    const OrbPlan p = orb_plan(w, h, nfeatures, caps);
    CHECK(p.rc == RELOC_OK, "rc %d (%s)", p.rc, p.err ? p.err : "");
    if (p.rc) return;
    const OrbTable &tab = p.tab;
    // levels: 256-byte aligned, disjoint, within the pyramid buffer of this capacity
    int64_t end = 0;
    int quota = 0;
    for (int l = 0; l < NLEV; ++l) {
        const OrbLevel &L = tab.lev[l];
        CHECK(L.w >= 1 && L.h >= 1 && L.stride % 64 == 0 && L.stride >= L.w, "level %d: %dx%d stride %d", l, L.w, L.h, L.stride);
        CHECK(L.stride <= 65535 && L.h <= 65535, "level %d does not fit uint16 coordinates", l);
        CHECK(L.off % 256 == 0 && L.off >= end, "level %d at %lld, the one before ends at %lld", l, (long long)L.off, (long long)end);
        end = L.off + (int64_t)L.stride * L.h;
        quota += L.quota;
    }
    CHECK((end + 255) / 256 * 256 <= caps.pyr_bytes, "pyramid of %lld bytes, buffer of %lld", (long long)end, (long long)caps.pyr_bytes);
    CHECK(quota == nfeatures, "quotas sum to %d", quota);
    // blocks
    const int ntx = (w + PT_W - 1) / PT_W, nty = (h + PT_H - 1) / PT_H;
    CHECK((int64_t)p.rz.size() <= caps.rz_entries, "%zu resize entries, room for %lld", p.rz.size(), (long long)caps.rz_entries);
    CHECK((int64_t)p.tiles.size() <= caps.tiles && (int)p.tiles.size() == ntx * nty, "%zu tiles, room for %lld", p.tiles.size(),
          (long long)caps.tiles);
    if ((int)p.tiles.size() != ntx * nty) return;
    // resize tables: taps inside the level below
    for (int l = 1; l < NLEV; ++l) {
        const OrbLevel &S = tab.lev[l - 1], &D = tab.lev[l];
        for (int a = 0; a < 2; ++a) {
            const int n = a ? D.h : D.w, sn = a ? S.h : S.w, o = tab.rz_off[l][2 * a], c = tab.rz_off[l][2 * a + 1];
            CHECK(o >= 0 && c == o + n && (size_t)(c + n) <= p.rz.size(), "level %d axis %d: table slices at %d, %d", l, a, o, c);
            for (int d = 0; d < n; ++d)
                CHECK(p.rz[o + d] >= 0 && p.rz[o + d] < sn && p.rz[c + d] >= 0 && p.rz[c + d] <= (1 << RELOC_RESIZE_COEF_BITS) &&
                          p.rz[o + d] < 65536, "level %d axis %d entry %d: offset %d coefficient %d", l, a, d, p.rz[o + d], p.rz[c + d]);
        }
    }
    // The stored rectangles cover a level exactly once.  Shown without a counter per pixel: every tile's rectangle is the
    // product of its grid column's x span and its grid row's y span (or empty where one of them is), and the spans of the
    // columns partition the stored width, those of the rows the height.
    int lds_need[NLEV] = {}, tab_need = 0;
    for (int l = 0; l < NLEV; ++l) {
        const OrbLevel &L = tab.lev[l];
        const int cols = l == 0 ? (L.w + 3) / 4 * 4 : L.stride;       // level 0 is stored to ceil4(w), the others with their padding
        std::vector<Span> X(ntx), Y(nty);
        for (int t = 0; t < ntx * nty; ++t) {
            const uint16_t *o = p.tiles[t].o[l];
            if (empty_rect(o)) continue;
            Span &x = X[t % ntx], &y = Y[t / ntx];
            if (!x.set) { x.a = o[0]; x.b = o[1]; x.set = true; }
            if (!y.set) { y.a = o[2]; y.b = o[3]; y.set = true; }
        }
        CHECK(partitions(X, cols), "level %d: the column spans do not partition 0..%d", l, cols);
        CHECK(partitions(Y, L.h), "level %d: the row spans do not partition 0..%d", l, L.h);
        for (int t = 0; t < ntx * nty; ++t) {
            const PyrTile &T = p.tiles[t];
            const uint16_t *o = T.o[l], *n = T.n[l];
            const Span &x = X[t % ntx], &y = Y[t / ntx];
            if (x.set && y.set) CHECK(o[0] == x.a && o[1] == x.b && o[2] == y.a && o[3] == y.b, "level %d tile %d is not column x row", l, t);
            else CHECK(o[0] == 0 && o[1] == 0 && o[2] == 0 && o[3] == 0, "level %d tile %d stores outside the grid", l, t);
            CHECK(o[0] % 4 == 0 && n[0] % 4 == 0 && o[1] % 4 == 0, "level %d tile %d: x0 %d / %d, stored x1 %d", l, t, o[0], n[0], o[1]);
            CHECK(n[0] <= n[1] && n[2] <= n[3] && n[1] <= L.w && n[3] <= L.h, "level %d tile %d: computed %d..%d x %d..%d", l, t, n[0], n[1], n[2], n[3]);
            // the tile's own pixels inside the image
            const int ox1 = o[1] < L.w ? o[1] : L.w;
            if (o[0] < ox1 && o[2] < o[3])
                CHECK(n[0] <= o[0] && n[1] >= ox1 && n[2] <= o[2] && n[3] >= o[3], "level %d tile %d: own pixels outside the computed rectangle", l, t);
            // the bilinear taps of the level above, clipped to this level as the kernel clips them
            if (l + 1 < NLEV && !empty_rect(T.n[l + 1])) {
                const uint16_t *u = T.n[l + 1];
                const int32_t *xo = p.rz.data() + tab.rz_off[l + 1][0], *yo = p.rz.data() + tab.rz_off[l + 1][2];
                for (int d = u[0]; d < u[1]; ++d) {
                    const int k0 = xo[d], k1 = k0 + 1 < L.w ? k0 + 1 : L.w - 1;
                    CHECK(n[0] <= k0 && k1 < n[1], "level %d tile %d: x taps %d, %d of column %d above outside %d..%d", l, t, k0, k1, d, n[0], n[1]);
                }
                for (int d = u[2]; d < u[3]; ++d) {
                    const int k0 = yo[d], k1 = k0 + 1 < L.h ? k0 + 1 : L.h - 1;
                    CHECK(n[2] <= k0 && k1 < n[3], "level %d tile %d: y taps %d, %d of row %d above outside %d..%d", l, t, k0, k1, d, n[2], n[3]);
                }
            }
            const int bytes = pitch_of(n) * (n[3] - n[2]);
            lds_need[l] = bytes > lds_need[l] ? bytes : lds_need[l];
        }
    }
    for (const PyrTile &T : p.tiles) {
        int words = 0;
        for (int l = 1; l < NLEV; ++l) words += (T.n[l][1] - T.n[l][0]) + (T.n[l][3] - T.n[l][2]);
        tab_need = words > tab_need ? words : tab_need;
    }
    // LDS: the level buffers in order, disjoint, each as large as any tile needs; then the table slices; 64 KB in all
    for (int l = 0; l < NLEV; ++l) {
        const int next = l + 1 < NLEV ? p.lds.lev[l + 1] : p.lds.tabs;
        CHECK(p.lds.lev[l] >= 0 && p.lds.lev[l] % 4 == 0 && next - p.lds.lev[l] >= lds_need[l], "LDS level %d: %d bytes at %d, %d needed", l,
              next - p.lds.lev[l], p.lds.lev[l], lds_need[l]);
    }
    CHECK(p.lds.tabs % 4 == 0 && p.lds_bytes - p.lds.tabs >= 4 * tab_need, "LDS tables: %d bytes, %d needed", p.lds_bytes - p.lds.tabs, 4 * tab_need);
    CHECK(p.lds_bytes <= PYR_LDS_MAX, "%d bytes of LDS", p.lds_bytes);
    if (p.lds_bytes > g_max_lds) { g_max_lds = p.lds_bytes; g_max_w = w; g_max_h = h; }
}

int main(int argc, char **argv)
{
    if (argc == 4 && !strcmp(argv[1], "levels")) {
        const int w = atoi(argv[2]), h = atoi(argv[3]);
        const OrbPlan p = orb_plan(w, h, 500, orb_caps(w, h));
        if (p.rc) { printf("rc %d (%s)\n", p.rc, p.err); return 1; }
        for (int l = 0; l < NLEV; ++l) printf("%d %d\n", p.tab.lev[l].w, p.tab.lev[l].h);
        return 0;
    }
    const int hs[4] = {64, 97, 480, 720}, ws[4] = {64, 333, 640, 1280};
    int sizes = 0;
    auto visit = [&](int w, int h) { check_size(w, h, 500); ++sizes; };
    for (int w = 64; w <= 1344; ++w)
        for (int h : hs) visit(w, h);
    for (int h = 64; h <= 800; ++h)
        for (int w : ws) visit(w, h);
    printf("sizes %d failures %d max_lds_bytes %d at %dx%d\n", sizes, g_failures, g_max_lds, g_max_w, g_max_h);
    return g_failures ? 1 : 0;
}
