// block_layout_check.cpp -- the carve arithmetic of a device block (csrc/reloc_block_layout.h) on the CPU.
//   block_layout_check          sweeps carve lists of 1..8 entries (element sizes 1, 2, 4, 8, 16; counts 0..67; alignment natural,
//                               16, 256): all lists of one and two entries, 200000 drawn ones of every longer length; then the
//                               sparse and dense stereo lists at three capacities each.  Last line: "lists N failures F".
// Asserted of every list: the sizing walk writes through no destination; it and the committing walk give the same offsets;
// every range starts at a multiple of max(alignof(T), ALIGN); the ranges lie in list order and are disjoint; the size
// returned is the end of the last range.  Of the stereo lists also: no range is less aligned than the hand-written offset it
// replaces.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../nclt-slam-project_amd/csrc/reloc_block_layout.h"

struct alignas(16) V16 { uint8_t b[16]; };
static_assert(sizeof(V16) == 16 && alignof(V16) == 16 && alignof(uint64_t) == 8, "element types of the sweep");

static const size_t SIZES[5] = {1, 2, 4, 8, 16};
static const size_t ALIGNS[3] = {1, 16, 256};
static const uintptr_t SENTINEL = (uintptr_t)0x5A5A5A5A5A5A5A5Aull;

struct Entry { int type, align, count; };
// one destination of every element type; an entry uses the one of its type
struct Dest {
    uint8_t *p1; uint16_t *p2; uint32_t *p4; uint64_t *p8; V16 *p16;
    void fill() { p1 = (uint8_t *)SENTINEL; p2 = (uint16_t *)SENTINEL; p4 = (uint32_t *)SENTINEL; p8 = (uint64_t *)SENTINEL; p16 = (V16 *)SENTINEL; }
    bool untouched() const
    {
        return (uintptr_t)p1 == SENTINEL && (uintptr_t)p2 == SENTINEL && (uintptr_t)p4 == SENTINEL && (uintptr_t)p8 == SENTINEL && (uintptr_t)p16 == SENTINEL;
    }
    uintptr_t get(int type) const
    {
        return type == 0 ? (uintptr_t)p1 : type == 1 ? (uintptr_t)p2 : type == 2 ? (uintptr_t)p4 : type == 3 ? (uintptr_t)p8 : (uintptr_t)p16;
    }
};

template <size_t ALIGN>
static void carve_type(BlockCarver &c, Dest &d, const Entry &e)
{
    switch (e.type) {
    case 0: c.aligned<ALIGN>(d.p1, e.count); break;
    case 1: c.aligned<ALIGN>(d.p2, e.count); break;
    case 2: c.aligned<ALIGN>(d.p4, e.count); break;
    case 3: c.aligned<ALIGN>(d.p8, e.count); break;
    default: c.aligned<ALIGN>(d.p16, e.count); break;
    }
}
// the natural alignment goes through operator(), 256 through own(): the spellings the library uses
static void carve(BlockCarver &c, Dest &d, const Entry &e)
{
    if (e.align == 1) { carve_type<16>(c, d, e); return; }
    if (e.align == 0)
        switch (e.type) {
        case 0: c(d.p1, e.count); return;
        case 1: c(d.p2, e.count); return;
        case 2: c(d.p4, e.count); return;
        case 3: c(d.p8, e.count); return;
        default: c(d.p16, e.count); return;
        }
    switch (e.type) {
    case 0: c.own(d.p1, e.count); return;
    case 1: c.own(d.p2, e.count); return;
    case 2: c.own(d.p4, e.count); return;
    case 3: c.own(d.p8, e.count); return;
    default: c.own(d.p16, e.count); return;
    }
}

static long g_lists = 0, g_failures = 0;
static uint8_t *g_buf = nullptr;      // 256-byte aligned, large enough for every list of the sweep
static const size_t BUF_BYTES = 8 * (67 * 16 + 256) + 256;

static void fail(const Entry *list, int n, const char *what)
{
    if (++g_failures > 20) return;
    printf("FAIL %s:", what);
    for (int k = 0; k < n; ++k) printf(" (size %zu align %zu count %d)", SIZES[list[k].type], ALIGNS[list[k].align], list[k].count);
    printf("\n");
}

static void check_list(const Entry *list, int n)
{
    ++g_lists;
    Dest d[8];
    size_t off_size[8], off_commit[8];
    // the sizing walk: offsets from `at` in front of each line's own bytes, no destination written
    for (int k = 0; k < n; ++k) d[k].fill();
    BlockCarver size;
    for (int k = 0; k < n; ++k) {
        carve(size, d[k], list[k]);
        off_size[k] = size.at - (size_t)list[k].count * SIZES[list[k].type];
    }
    for (int k = 0; k < n; ++k)
        if (!d[k].untouched()) { fail(list, n, "the sizing walk wrote a destination"); return; }
    if (size.at > BUF_BYTES) { fail(list, n, "the list outgrows the check's buffer"); return; }
    BlockCarver commit{g_buf};
    for (int k = 0; k < n; ++k) carve(commit, d[k], list[k]);
    if (commit.at != size.at) { fail(list, n, "the two walks disagree on the size"); return; }
    size_t end = 0;
    for (int k = 0; k < n; ++k) {
        const size_t a = SIZES[list[k].type] > ALIGNS[list[k].align] ? SIZES[list[k].type] : ALIGNS[list[k].align];
        off_commit[k] = (size_t)(d[k].get(list[k].type) - (uintptr_t)g_buf);
        if (off_commit[k] != off_size[k]) { fail(list, n, "the two walks disagree on an offset"); return; }
        if (off_commit[k] % a || d[k].get(list[k].type) % a) { fail(list, n, "a range is misaligned"); return; }
        if (off_commit[k] < end) { fail(list, n, "a range starts inside the one before it"); return; }
        if (off_commit[k] - end >= a) { fail(list, n, "a gap of a whole alignment step"); return; }
        end = off_commit[k] + (size_t)list[k].count * SIZES[list[k].type];
    }
    if (end != size.at) { fail(list, n, "the size is not the end of the last range"); return; }
}

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static unsigned draw(unsigned n)
{
    g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
    return (unsigned)((g_rng >> 33) % n);
}

// ---- the stereo lists ------------------------------------------------------------------------------------------------------
struct alignas(8) U2 { uint32_t x, y; };      // HIP's uint2
struct Sparse { float *disp; uint16_t *mm; uint8_t *status; uint8_t *plane; };
struct Dense { U2 *best; uint32_t *rmap; float *disp; uint16_t *mm; uint8_t *status; uint8_t *left; };

static size_t align_of_offset(size_t x)
{
    size_t a = 256;
    while (x % a) a /= 2;
    return a;
}

struct Range { const char *name; uintptr_t p; size_t bytes, elem, old_off; };

// ranges in list order: in the block, aligned for their type and no less than the old offset, disjoint
static void check_ranges(const char *what, long a, long b, const uint8_t *base, size_t total, const Range *r, int n)
{
    ++g_lists;
    size_t end = 0;
    for (int k = 0; k < n; ++k) {
        const size_t off = (size_t)(r[k].p - (uintptr_t)base);
        const bool ok = off >= end && off % r[k].elem == 0 && align_of_offset(off) >= align_of_offset(r[k].old_off) && off + r[k].bytes <= total;
        if (!ok) {
            ++g_failures;
            printf("FAIL %s %ld %ld: %s at %zu (%zu bytes), the range before ends at %zu, the hand offset was %zu, block %zu\n", what, a, b,
                   r[k].name, off, r[k].bytes, end, r[k].old_off, total);
        }
        end = off + r[k].bytes;
    }
    if (end != total) { ++g_failures; printf("FAIL %s %ld %ld: size %zu, last range ends at %zu\n", what, a, b, total, end); }
}

static void check_stereo(int w, int h, int mf)
{
    const int64_t px = (int64_t)w * h;
    {
        Sparse s;
        memset(&s, 0x5A, sizeof(s));
        Sparse before = s;
        BlockCarver size;
        stereo_sparse_lines(size, s, mf, px);
        if (memcmp(&s, &before, sizeof(s))) { ++g_failures; printf("FAIL sparse %d %ld: the sizing walk wrote a destination\n", mf, (long)px); }
        uint8_t *base = (uint8_t *)aligned_alloc(256, (size.at + 255) / 256 * 256);
        BlockCarver commit{base};
        stereo_sparse_lines(commit, s, mf, px);
        if (commit.at != size.at) { ++g_failures; printf("FAIL sparse: the two walks disagree on the size\n"); }
        const size_t m = (size_t)mf;
        const Range r[4] = {{"disp", (uintptr_t)s.disp, m * 4, 4, 0}, {"mm", (uintptr_t)s.mm, m * 2, 2, m * 4}, {"status", (uintptr_t)s.status, m, 1, m * 6},
                            {"plane", (uintptr_t)s.plane, (size_t)px, 1, (m * 7 + 255) / 256 * 256}};
        check_ranges("sparse", mf, (long)px, base, size.at, r, 4);
        free(base);
    }
    {
        Dense d;
        memset(&d, 0x5A, sizeof(d));
        Dense before = d;
        BlockCarver size;
        stereo_dense_lines(size, d, px);
        if (memcmp(&d, &before, sizeof(d))) { ++g_failures; printf("FAIL dense %ld: the sizing walk wrote a destination\n", (long)px); }
        uint8_t *base = (uint8_t *)aligned_alloc(256, (size.at + 255) / 256 * 256);
        BlockCarver commit{base};
        stereo_dense_lines(commit, d, px);
        if (commit.at != size.at) { ++g_failures; printf("FAIL dense: the two walks disagree on the size\n"); }
        const size_t p = (size_t)px;
        const Range r[6] = {{"best", (uintptr_t)d.best, p * 8, 8, 0}, {"rmap", (uintptr_t)d.rmap, p * 4, 4, p * 8}, {"disp", (uintptr_t)d.disp, p * 4, 4, p * 12},
                            {"mm", (uintptr_t)d.mm, p * 2, 2, p * 16}, {"status", (uintptr_t)d.status, p, 1, p * 18}, {"left", (uintptr_t)d.left, p, 1, p * 19}};
        check_ranges("dense", w, h, base, size.at, r, 6);
        free(base);
    }
}

int main()
{
    g_buf = (uint8_t *)aligned_alloc(256, (BUF_BYTES + 255) / 256 * 256);
    if (!g_buf) { printf("no memory\n"); return 2; }
    Entry list[8];
    // every list of one entry and of two
    for (int t0 = 0; t0 < 5; ++t0)
        for (int a0 = 0; a0 < 3; ++a0)
            for (int c0 = 0; c0 <= 67; ++c0) {
                list[0] = {t0, a0, c0};
                check_list(list, 1);
                for (int t1 = 0; t1 < 5; ++t1)
                    for (int a1 = 0; a1 < 3; ++a1)
                        for (int c1 = 0; c1 <= 67; ++c1) {
                            list[1] = {t1, a1, c1};
                            check_list(list, 2);
                        }
            }
    // drawn lists of 3..8 entries; every (size, alignment, count) stands once at every position of every length
    for (int n = 3; n <= 8; ++n) {
        for (int pos = 0; pos < n; ++pos)
            for (int t = 0; t < 5; ++t)
                for (int a = 0; a < 3; ++a)
                    for (int c = 0; c <= 67; ++c) {
                        for (int k = 0; k < n; ++k) list[k] = {(int)draw(5), (int)draw(3), (int)draw(68)};
                        list[pos] = {t, a, c};
                        check_list(list, n);
                    }
        for (int it = 0; it < 200000; ++it) {
            for (int k = 0; k < n; ++k) list[k] = {(int)draw(5), (int)draw(3), (int)draw(68)};
            check_list(list, n);
        }
    }
    static const int WH[3][2] = {{64, 64}, {97, 65}, {1280, 720}};
    static const int MF[3] = {64, 513, 8192};
    for (const auto &wh : WH)
        for (int mf : MF) check_stereo(wh[0], wh[1], mf);
    free(g_buf);
    printf("lists %ld failures %ld\n", g_lists, g_failures);
    return g_failures ? 1 : 0;
}
