// frame_layout.hpp -- the kernel-written buffers of one frame: which there are, how many elements each holds, and how a frame's share
// of one allocation is cut into them.  Host code only, no HIP calls: renderer.cpp sizes, sums and carves through this one list.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "device_types.hpp"

namespace swfr {

inline size_t pad256(size_t bytes) { return (bytes + 255) & ~size_t(255); }   // every carved piece starts on a 256-byte boundary

// The eight numbers the sizes depend on, and the element counts that follow from them.
struct FrameDims {
    size_t n_edges = 0, n_paths = 0, n_slots = 0, n_rows = 0, n_chunks = 0, n_strips = 0, n_strip_slots = 0, cell_total = 0;
    // from what layout_scene worked out (a SceneLayout) and the sizes of the arrays the device gets
    template <class Layout>
    static FrameDims of_layout(const Layout& L, size_t n_edges, size_t n_paths) {
        return FrameDims{n_edges, n_paths, L.n_slots, L.n_rows, L.n_chunks, L.n_strips, L.n_strip_slots, L.cell_total};
    }

    size_t edge_count() const { return 2 * n_edges + 1; }
    size_t band_entry_count() const { return n_slots; }
    size_t row_count() const { return n_slots * TILE_H + 64; }
    size_t cell_count() const { return cell_total; }
    size_t slow_count() const { return 2 * (n_rows + 64); }       // (slow and huge, two queues each: a pass reads one and refills the other)
    size_t path_word_count() const { return n_paths + 64; }       // (path_flag and path_queue)
    size_t chunk_count() const { return n_chunks + 1; }
    size_t band_slot_count() const { return n_slots + 8; }
    size_t strip_count() const { return n_strip_slots + 1; }
    size_t strip_cost_count() const { return n_strips + 1; }
};

// THE list of a frame's kernel-written buffers: v(member of f, element count, per parity) once per buffer, in the order they are
// carved.  Every sum of sizes and every carve goes through here, so the two cannot disagree.
// per parity: k2_bin writes or clears the buffer.  A frame set that bins its next frame beside the row pass of the one before
// (k2_rows_ahead_b) has two descriptors, parity 0 and 1, with a copy of their own of each such buffer; what only the row and tile
// passes write -- rows, cells, the two row queues, path_queue -- is one buffer both descriptors point to (carve_frame_ahead).
template <class V>
void for_each_frame_buffer_parity(Frame2& f, const FrameDims& d, V&& v) {
    v(f.edges, d.edge_count(), true); v(f.band_list, d.band_entry_count(), true); v(f.rows, d.row_count(), false); v(f.cells, d.cell_count(), false);
    v(f.slow, d.slow_count(), false); v(f.huge, d.slow_count(), false); v(f.path_flag, d.path_word_count(), true); v(f.path_queue, d.path_word_count(), false);
    v(f.chunks, d.chunk_count(), true); v(f.band_slots, d.band_slot_count(), true); v(f.strips, d.strip_count(), true); v(f.strip_cost, d.strip_cost_count(), true);
    v(f.counters, size_t(C2_WORDS), true);
}
// ... as v(member of f, element count)
template <class V>
void for_each_frame_buffer(Frame2& f, const FrameDims& d, V&& v) {
    for_each_frame_buffer_parity(f, d, [&](auto*& p, size_t n, bool) { v(p, n); });
}
// points f's buffers into the bytes from `base` on and returns their end: the next frame's base
inline uint8_t* carve_frame(Frame2& f, const FrameDims& d, uint8_t* base) {
    for_each_frame_buffer(f, d, [&](auto*& p, size_t n) { p = reinterpret_cast<decltype(p + 0)>(base); base += pad256(n * sizeof(*p)); });
    return base;
}
// bytes of one frame's buffers in a carved allocation: what carve_frame advances by
inline size_t frame_work_bytes(const FrameDims& d) {
    Frame2 f{};
    size_t bytes = 0;
    for_each_frame_buffer(f, d, [&](auto* p, size_t n) { bytes += pad256(n * sizeof(*p)); });
    return bytes;
}

// The other parity's descriptor of a frame set.  f is a copy of the parity-0 descriptor: its per-parity buffers are pointed into the
// bytes from `base` on (the end is returned), the shared ones stay where parity 0 has them.
inline uint8_t* carve_frame_ahead(Frame2& f, const FrameDims& d, uint8_t* base) {
    for_each_frame_buffer_parity(f, d, [&](auto*& p, size_t n, bool per_parity) {
        if (per_parity) { p = reinterpret_cast<decltype(p + 0)>(base); base += pad256(n * sizeof(*p)); }
    });
    return base;
}
// bytes of the other parity's own buffers: what carve_frame_ahead advances by
inline size_t frame_ahead_bytes(const FrameDims& d) {
    Frame2 f{};
    size_t bytes = 0;
    for_each_frame_buffer_parity(f, d, [&](auto* p, size_t n, bool per_parity) { if (per_parity) bytes += pad256(n * sizeof(*p)); });
    return bytes;
}

// The class bytes of a frame and, behind them (16-byte aligned), one StripTop record per strip of the handle: both are cleared when a
// scene is uploaded (the tile pass clears a strip's record again when it has read it).
inline size_t cls_bytes_of(size_t n_slots, size_t tiles_x) { return (size_t(STRIPS_PER_TILE) * n_slots * tiles_x + 64 + 15) & ~size_t(15); }
inline size_t cls_region_bytes(size_t n_slots, size_t tiles_x, size_t n_strips) { return cls_bytes_of(n_slots, tiles_x) + (n_strips + 1) * sizeof(StripTop); }
inline size_t cls_region_bytes(const FrameDims& d, size_t tiles_x) { return cls_region_bytes(d.n_slots, tiles_x, d.n_strips); }
// f.cls and f.strip_top of a region of cls_region_bytes(d, tiles_x) at base
inline void set_cls_region(Frame2& f, const FrameDims& d, size_t tiles_x, uint8_t* base) {
    f.cls = base;
    f.strip_top = reinterpret_cast<StripTop*>(base + cls_bytes_of(d.n_slots, tiles_x));
}

}  // namespace swfr
