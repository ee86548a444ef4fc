// reloc_block_layout.h -- the offset arithmetic of a device block (DevBlock, reloc_internal.h): a block's layout is a list of
// carve lines in block order, each one `count` elements of the destination's type at the next multiple of its alignment.
// Plain C++ without HIP: the library walks a list twice (DevBlock::layout), tests/host/block_layout_check.cpp sweeps the
// arithmetic on the CPU.  The lists of the two stereo blocks stand here as well, over any struct with their members, so that
// the same program evaluates them.
#pragma once
#include <stddef.h>
#include <stdint.h>

constexpr size_t BLOCK_ALIGN = 256;      // what the device allocator aligns a block to, and so every buffer that once was a block of its own

// One walk over a carve list.  The sizing walk (base == NULL) computes offsets only and writes through no destination; the
// committing walk assigns base + offset.  Both advance `at` alike: behind the list it is the bytes the list takes.
struct BlockCarver {
    uint8_t *base = nullptr;
    size_t at = 0;
    // count elements of T at the next multiple of max(alignof(T), ALIGN)
    template <size_t ALIGN, typename T>
    void aligned(T *&dst, int64_t count)
    {
        constexpr size_t A = ALIGN > alignof(T) ? ALIGN : alignof(T);
        static_assert(A % alignof(T) == 0 && BLOCK_ALIGN % A == 0, "an alignment divides the block's");
        at = (at + A - 1) / A * A;
        if (base) dst = reinterpret_cast<T *>(base + at);
        at += (size_t)(count > 0 ? count : 0) * sizeof(T);
    }
    template <typename T>
    void operator()(T *&dst, int64_t count) { aligned<1>(dst, count); }      // natural alignment
    template <typename T>
    void own(T *&dst, int64_t count) { aligned<BLOCK_ALIGN>(dst, count); }   // a buffer aligned like a block of its own
};

// Sparse stereo (StereoState): disparities, millimetres, status of max_feat keypoints, then the right eye's plain gray plane of
// px = max_w * max_h bytes on a 256-byte boundary; what lies in front of the plane is zeroed on the first enable.
template <typename S>
void stereo_sparse_lines(BlockCarver &c, S &s, int64_t max_feat, int64_t px)
{
    c.own(s.disp, max_feat);
    c.aligned<4>(s.mm, max_feat);
    c(s.status, max_feat);
    c.own(s.plane, px);
}

// Dense stereo (StereoState::Dense): six planes of px = max_w * max_h pixels
template <typename D>
void stereo_dense_lines(BlockCarver &c, D &d, int64_t px)
{
    c.own(d.best, px);
    c.aligned<8>(d.rmap, px);
    c(d.disp, px);
    c.aligned<16>(d.mm, px);
    c(d.status, px);
    c(d.left, px);
}

// Semi-global stereo (StereoState::Sgm): the cost volume and the sum volume of `entries` = w * h * num_disparities values, the
// best plane of px pixels
template <typename G>
void stereo_sgm_lines(BlockCarver &c, G &g, int64_t entries, int64_t px)
{
    c.own(g.sum, entries);
    c.own(g.vol, entries);
    c.own(g.best, px);
}

// Census stereo (StereoState::Census): the census planes of both eyes, px = max_w * max_h bytes each
template <typename C>
void stereo_census_lines(BlockCarver &c, C &s, int64_t px)
{
    c.own(s.left, px);
    c.own(s.right, px);
}
