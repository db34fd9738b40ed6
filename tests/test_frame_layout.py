"""csrc/frame_layout.hpp: the one list of a frame's kernel-written buffers, their element counts, and the carve of one allocation into
them.  No GPU: a stand-alone C++ program includes the header, carves real memory for several FrameDims and checks the regions; it is
built with the host g++ and run, once plainly and once under AddressSanitizer and UBSan."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "swf_renderer_amd", "csrc")

# The literals: worked out by hand from the formulas renderer.cpp spelled out before this header existed (COUNTER_WORDS = 32, TILE_H = 16,
# two strips per tile, sizeof(StripTop) = 16):
#   edges 2 n_edges + 1 | band_list n_slots | rows 16 n_slots + 64 | cells cell_total | slow, huge 2 (n_rows + 64) | path_flag, path_queue
#   n_paths + 64 | chunks n_chunks + 1 | band_slots n_slots + 8 | strips n_strip_slots + 1 | strip_cost n_strips + 1 | counters 32
#   class bytes (2 n_slots tiles_x + 64) rounded up to 16, + 16 (n_strips + 1) for the region
PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "frame_layout.hpp"
using namespace swfr;

static int failures = 0;
static void check(bool ok, const char* what, const char* set) { if (!ok) { ++failures; std::printf("FAIL [%s] %s\n", set, what); } }

struct Region { const char* name; uint8_t* at; size_t count, elem; size_t bytes() const { return count * elem; } };
static const char* NAMES[13] = {"edges", "band_list", "rows", "cells", "slow", "huge", "path_flag", "path_queue", "chunks", "band_slots",
                                "strips", "strip_cost", "counters"};
static std::vector<Region> regions_of(Frame2& f, const FrameDims& d) {
    std::vector<Region> out;
    for_each_frame_buffer(f, d, [&](auto* p, size_t n) {
        out.push_back(Region{out.size() < 13 ? NAMES[out.size()] : "?", reinterpret_cast<uint8_t*>(p), n, sizeof(*p)});
    });
    return out;
}
static uint8_t* aligned(std::vector<uint8_t>& store, size_t bytes) {
    store.assign(bytes + 256, 0xee);
    return store.data() + (256 - reinterpret_cast<uintptr_t>(store.data()) % 256) % 256;
}

// frames carved back to back into one allocation, as a batch group does; every region is then written from end to end
static void carve_and_check(const char* set, const std::vector<FrameDims>& dims, size_t tiles_x) {
    size_t work_bytes = 0, cls_total = 0;
    for (const FrameDims& d : dims) { work_bytes += frame_work_bytes(d); cls_total += pad256(cls_region_bytes(d, tiles_x)); }
    std::vector<uint8_t> work_store, cls_store;
    uint8_t* const base = aligned(work_store, work_bytes);
    uint8_t* const cls_base = aligned(cls_store, cls_total);
    std::vector<Frame2> frames(dims.size());
    std::vector<Region> all;
    uint8_t *w = base, *c = cls_base;
    for (size_t k = 0; k < dims.size(); ++k) {
        const FrameDims& d = dims[k];
        Frame2& f = frames[k];
        std::memset(&f, 0, sizeof f);
        uint8_t* const end = carve_frame(f, d, w);
        check(end == w + frame_work_bytes(d), "carve_frame advances by frame_work_bytes", set);
        const std::vector<Region> regs = regions_of(f, d);
        check(regs.size() == 13, "thirteen buffers", set);
        uint8_t* cursor = w;
        for (const Region& g : regs) {
            check(reinterpret_cast<uintptr_t>(g.at) % 256 == 0, "a region is 256-byte aligned", set);
            check(g.at == cursor, "the regions follow in the enumeration's order, each behind the one before", set);
            cursor = g.at + pad256(g.bytes());
            all.push_back(g);
        }
        check(cursor == end, "the last region of a frame ends where the next frame begins", set);
        w = end;
        set_cls_region(f, d, tiles_x, c);
        uint8_t* const top = reinterpret_cast<uint8_t*>(f.strip_top);
        const size_t region = cls_region_bytes(d, tiles_x);
        check(f.cls == c, "cls starts its region", set);
        check(top >= c + size_t(STRIPS_PER_TILE) * d.n_slots * tiles_x + 64, "strip_top lies behind the class bytes", set);
        check(reinterpret_cast<uintptr_t>(top) % 16 == 0, "strip_top is 16-byte aligned", set);
        check(top + (d.n_strips + 1) * sizeof(StripTop) == c + region, "the StripTop records end the cls region", set);
        std::memset(f.cls, int(k + 1), region);
        c += pad256(region);
    }
    check(w == base + work_bytes, "the last region ends exactly at base + work_bytes", set);
    check(c == cls_base + cls_total, "the cls regions end at the sum of their padded sizes", set);
    for (size_t i = 0; i < all.size(); ++i)
        for (size_t j = i + 1; j < all.size(); ++j)
            check(all[i].at + all[i].bytes() <= all[j].at || all[j].at + all[j].bytes() <= all[i].at, "regions are pairwise disjoint", set);
    // every region filled with its own number, then read back: none has run into another (and none leaves the allocation: ASan)
    for (size_t i = 0; i < all.size(); ++i) std::memset(all[i].at, int(i % 251) + 1, all[i].bytes());
    for (size_t i = 0; i < all.size(); ++i)
        for (size_t b = 0; b < all[i].bytes(); ++b)
            if (all[i].at[b] != uint8_t(i % 251 + 1)) { check(false, "a region was overwritten by another", set); break; }
}

static void check_counts(const char* set, const FrameDims& d, const size_t (&want)[13], size_t tiles_x, size_t cls_bytes, size_t cls_region) {
    Frame2 f{};
    const std::vector<Region> regs = regions_of(f, d);
    for (size_t i = 0; i < regs.size() && i < 13; ++i)
        if (regs[i].count != want[i]) { ++failures; std::printf("FAIL [%s] %s holds %zu elements, expected %zu\n", set, regs[i].name, regs[i].count, want[i]); }
    check(cls_bytes_of(d.n_slots, tiles_x) == cls_bytes, "cls_bytes_of", set);
    check(cls_region_bytes(d, tiles_x) == cls_region && cls_region_bytes(d.n_slots, tiles_x, d.n_strips) == cls_region, "cls_region_bytes", set);
}

struct LayoutLike { size_t n_slots, n_rows, n_chunks, n_strips, n_strip_slots, cell_total; };

int main() {
    FrameDims empty;                                                   // all zeros
    FrameDims one;    one.n_edges = 1; one.n_paths = 1; one.n_slots = 1; one.n_rows = 1; one.n_chunks = 1; one.n_strips = 2; one.n_strip_slots = 16; one.cell_total = 4100;
    FrameDims bare;   bare.n_edges = 12; bare.n_paths = 3; bare.n_slots = 5; bare.n_rows = 0; bare.n_chunks = 0; bare.n_strips = 0; bare.n_strip_slots = 0; bare.cell_total = 4096;
    const FrameDims mid = FrameDims::of_layout(LayoutLike{210, 3000, 95, 1360, 1536, 69632}, 1000, 37);
    check(mid.n_edges == 1000 && mid.n_paths == 37 && mid.n_slots == 210 && mid.n_rows == 3000 &&
          mid.n_chunks == 95 && mid.n_strips == 1360 && mid.n_strip_slots == 1536 && mid.cell_total == 69632, "of_layout reads the eight numbers", "mid");
    check(pad256(0) == 0 && pad256(1) == 256 && pad256(256) == 256 && pad256(257) == 512, "pad256", "pad");

    const size_t want_empty[13] = {1, 0, 64, 0, 128, 128, 64, 64, 1, 8, 1, 1, 32};
    const size_t want_one[13] = {3, 1, 80, 4100, 130, 130, 65, 65, 2, 9, 17, 3, 32};
    const size_t want_mid[13] = {2001, 210, 3424, 69632, 6128, 6128, 101, 101, 96, 218, 1537, 1361, 32};
    check_counts("empty", empty, want_empty, 1, 64, 80);
    check_counts("one", one, want_one, 1, 80, 128);
    check_counts("mid", mid, want_mid, 5, 2176, 23952);

    carve_and_check("empty", {empty}, 1);
    carve_and_check("one", {one}, 1);
    carve_and_check("bare", {bare}, 3);
    carve_and_check("mid", {mid}, 5);
    carve_and_check("group", {mid, empty, one, bare, mid}, 5);
    if (failures) { std::printf("%d checks failed\n", failures); return 1; }
    std::printf("frame layout ok\n");
    return 0;
}
"""


def _build_and_run(tmp_path, name, extra):
    gxx = shutil.which("g++")
    assert gxx, "the host g++ is needed to check frame_layout.hpp"
    src = tmp_path / "frame_layout_check.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / name
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I" + CSRC] + extra + [str(src), "-o", str(exe)])
    run = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0 and "frame layout ok" in run.stdout, run.stdout


def test_carved_regions_and_element_counts(tmp_path):
    _build_and_run(tmp_path, "check", [])


def test_carve_runs_clean_under_asan_and_ubsan(tmp_path):
    """The same stand-alone program (nothing loaded into Python) with the sanitizers: every carved region is written end to end."""
    _build_and_run(tmp_path, "check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])


def test_header_is_plain_cxx():
    """frame_layout.hpp includes device_types.hpp and standard headers only, and makes no HIP calls."""
    text = open(os.path.join(CSRC, "frame_layout.hpp")).read()
    includes = [ln.split()[1] for ln in text.splitlines() if ln.startswith("#include")]
    assert includes == ["<stddef.h>", "<stdint.h>", '"device_types.hpp"']
    assert "hip" not in text.replace("HIP calls", "").lower()
