"""csrc/frame_layout.hpp, the two descriptors of a frame set that bins its next frame beside the row pass (parity 0 and 1): for seeded
FrameDims the parity-1 descriptor shares with parity 0 exactly rows, cells, slow, huge and path_queue; every other piece -- both
parities' -- is disjoint from every other, 256-byte aligned and inside the allocation, and frame_work_bytes + frame_ahead_bytes is
what the two carves advance by.  No GPU: a stand-alone C++ program includes the header and carves real memory; it is built with the
host g++ and run, once plainly and once under AddressSanitizer and UBSan."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "swf_renderer_amd", "csrc")

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "frame_layout.hpp"
using namespace swfr;

static int failures = 0;
static void check(bool ok, const char* what, unsigned set) { if (!ok) { ++failures; std::printf("FAIL [dims %u] %s\n", set, what); } }

struct Region { std::string name; uint8_t* at; size_t bytes; bool per_parity; };
static const char* NAMES[13] = {"edges", "band_list", "rows", "cells", "slow", "huge", "path_flag", "path_queue", "chunks", "band_slots",
                                "strips", "strip_cost", "counters"};
// what the two parities share: only the row and tile passes write these
static bool shared_name(const std::string& n) { return n == "rows" || n == "cells" || n == "slow" || n == "huge" || n == "path_queue"; }
static std::vector<Region> regions_of(Frame2& f, const FrameDims& d) {
    std::vector<Region> out;
    for_each_frame_buffer_parity(f, d, [&](auto* p, size_t n, bool per_parity) {
        out.push_back(Region{out.size() < 13 ? NAMES[out.size()] : "?", reinterpret_cast<uint8_t*>(p), n * sizeof(*p), per_parity});
    });
    return out;
}
static uint32_t rng_state = 12345u;
static uint32_t rnd(uint32_t below) { rng_state = rng_state * 1664525u + 1013904223u; return (rng_state >> 8) % below; }

static void one(unsigned set, const FrameDims& d, size_t tiles_x) {
    const size_t work_bytes = frame_work_bytes(d) + frame_ahead_bytes(d);
    const size_t cls_one = cls_region_bytes(d, tiles_x), cls_total = pad256(cls_one) + cls_one;
    std::vector<uint8_t> work_store(work_bytes + 256, 0xee), cls_store(cls_total + 256, 0xee);
    uint8_t* const base = work_store.data() + (256 - reinterpret_cast<uintptr_t>(work_store.data()) % 256) % 256;
    uint8_t* const cbase = cls_store.data() + (256 - reinterpret_cast<uintptr_t>(cls_store.data()) % 256) % 256;
    Frame2 f0, f1;
    std::memset(&f0, 0, sizeof f0);
    uint8_t* const mid = carve_frame(f0, d, base);
    set_cls_region(f0, d, tiles_x, cbase);
    f1 = f0;
    uint8_t* const end = carve_frame_ahead(f1, d, mid);
    set_cls_region(f1, d, tiles_x, cbase + pad256(cls_one));
    check(mid == base + frame_work_bytes(d), "carve_frame advances by frame_work_bytes", set);
    check(end == mid + frame_ahead_bytes(d), "carve_frame_ahead advances by frame_ahead_bytes", set);
    check(end == base + work_bytes, "the two carves end the allocation", set);
    const std::vector<Region> r0 = regions_of(f0, d), r1 = regions_of(f1, d);
    check(r0.size() == 13 && r1.size() == 13, "thirteen buffers", set);
    std::vector<Region> all;
    size_t ahead_sum = 0;
    for (size_t i = 0; i < r0.size() && i < r1.size(); ++i) {
        check(r0[i].per_parity == !shared_name(r0[i].name), "the list marks exactly what k2_bin writes as per parity", set);
        all.push_back(r0[i]);
        if (shared_name(r0[i].name)) check(r1[i].at == r0[i].at, (r0[i].name + " is shared by the parities").c_str(), set);
        else { check(r1[i].at != r0[i].at, (r0[i].name + " has a copy per parity").c_str(), set); all.push_back(r1[i]); ahead_sum += pad256(r1[i].bytes); }
        check(r1[i].bytes == r0[i].bytes, "both parities' buffers hold the same elements", set);
    }
    check(ahead_sum == frame_ahead_bytes(d), "frame_ahead_bytes is the sum of the per-parity buffers", set);
    check(reinterpret_cast<uint8_t*>(f1.cls) != reinterpret_cast<uint8_t*>(f0.cls) && f1.strip_top != f0.strip_top, "cls and strip_top have a copy per parity", set);
    for (const Region& g : all) {
        check(reinterpret_cast<uintptr_t>(g.at) % 256 == 0, "a piece is 256-byte aligned", set);
        check(g.at >= base && g.at + g.bytes <= base + work_bytes, "a piece lies inside the allocation", set);
    }
    for (size_t i = 0; i < all.size(); ++i)
        for (size_t j = i + 1; j < all.size(); ++j)
            check(all[i].at + all[i].bytes <= all[j].at || all[j].at + all[j].bytes <= all[i].at, "pieces are pairwise disjoint", set);
    // every piece filled with its own number, then read back: none has run into another (and none leaves the allocation: ASan)
    for (size_t i = 0; i < all.size(); ++i) std::memset(all[i].at, int(i % 251) + 1, all[i].bytes);
    for (size_t i = 0; i < all.size(); ++i)
        for (size_t b = 0; b < all[i].bytes; ++b)
            if (all[i].at[b] != uint8_t(i % 251 + 1)) { check(false, "a piece was overwritten by another", set); break; }
    // the two cls regions: each inside the allocation, disjoint, strip_top 16-byte aligned behind the class bytes
    uint8_t* const c0 = f0.cls; uint8_t* const c1 = f1.cls;
    check(c0 == cbase && c1 == cbase + pad256(cls_one) && c1 + cls_one <= cbase + cls_total, "the cls regions follow each other inside the allocation", set);
    check(reinterpret_cast<uintptr_t>(c1) % 256 == 0 && reinterpret_cast<uintptr_t>(f1.strip_top) % 16 == 0, "the second cls region is aligned", set);
    check(reinterpret_cast<uint8_t*>(f1.strip_top) + (d.n_strips + 1) * sizeof(StripTop) == c1 + cls_one, "the StripTop records end the second cls region", set);
    std::memset(c0, 1, cls_one); std::memset(c1, 2, cls_one);
    check(c0[cls_one - 1] == 1 && c1[0] == 2, "the cls regions do not overlap", set);
}

int main() {
    one(0, FrameDims{}, 1);
    for (unsigned s = 1; s <= 40; ++s) {
        FrameDims d;
        d.n_edges = rnd(5000); d.n_paths = rnd(700); d.n_slots = rnd(900); d.n_rows = rnd(20000); d.n_chunks = rnd(1200);
        d.n_strips = rnd(3000); d.n_strip_slots = d.n_strips + rnd(64); d.cell_total = rnd(200000);
        one(s, d, 1 + rnd(40));
    }
    if (failures) { std::printf("%d checks failed\n", failures); return 1; }
    std::printf("parity layout ok\n");
    return 0;
}
"""


def _build_and_run(tmp_path, name, extra):
    gxx = shutil.which("g++")
    assert gxx, "the host g++ is needed to check frame_layout.hpp"
    src = tmp_path / "parity_layout_check.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / name
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I" + CSRC] + extra + [str(src), "-o", str(exe)])
    run = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0 and "parity layout ok" in run.stdout, run.stdout


def test_the_parities_share_exactly_what_k2_bin_leaves_alone(tmp_path):
    _build_and_run(tmp_path, "check", [])


def test_the_parity_carve_runs_clean_under_asan_and_ubsan(tmp_path):
    """The same stand-alone program (nothing loaded into Python) with the sanitizers: every carved piece is written end to end."""
    _build_and_run(tmp_path, "check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
