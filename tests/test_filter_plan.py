"""csrc/filter_plan.hpp, the pass plan of a filter list: for both sources (the sub-frame's framebuffer, a bitmap's own texels) every list
of 1..SWFR_MAX_FILTERS entries drawn from 25 entry types -- 12 blurs of 0, 1, 2, 3, 4 and 6 box steps, the same 12 as shadows with the
inner flag alternating, one convolution -- is planned, and the plan interpreted over symbolic buffer contents (a hash per buffer; a
step writes the hash of its op, its entry and what it read).  The sequential model f_n(... f_1(group)) is written out here pass by
pass, without the planner: the k-th pass of a plan must write the model's k-th value, so no step reads a buffer an earlier step has
overwritten with something else, and T0 ends holding the model's result.  Beside that: no read of a buffer nothing wrote, no step in
place but a shadow's finish pass, the framebuffer never written, `uses` exactly the buffers named, and the step counts -- no pass, no
copy more than the entries ask for.  No GPU: a stand-alone C++ program includes the header; it is built with the host g++ and run, once
plainly and once under AddressSanitizer and UBSan."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "swf_renderer_amd", "csrc")

PROGRAM = r"""
#include <cstdio>
#include <cstdint>
#include <vector>
#include "filter_plan.hpp"
using namespace swfr;

static int failures = 0;
static const char* BUF[4] = {"FB", "T0", "T1", "T2"};
static const char* OPS[7] = {"CAPTURE", "BOX_H", "BOX_V", "SHADOW_ALPHA", "SHADOW_FINISH", "CONVOLVE", "COPY"};
static void describe(const swfr_filter* list, uint32_t n, Source source, const FilterPlan& P) {
    std::printf("  %s:", source == Source::Framebuffer ? "framebuffer" : "texels");
    for (uint32_t i = 0; i < n; ++i) std::printf(" [kind %u box %u x %u passes %u]", list[i].kind, list[i].shadow.blur_x, list[i].shadow.blur_y, list[i].shadow.passes);
    std::printf("\n");
    for (uint32_t k = 0; k < P.n; ++k)
        std::printf("    %s %s -> %s group %s entry %u\n", OPS[int(P.steps[k].op)], BUF[P.steps[k].src], BUF[P.steps[k].dst], BUF[P.steps[k].group], unsigned(P.steps[k].entry));
}
struct Checker {
    const swfr_filter* list; uint32_t n; Source source; const FilterPlan& P; bool told = false;
    void operator()(bool ok, const char* what) {
        if (ok) return;
        ++failures;
        if (failures > 20) return;
        std::printf("FAIL %s\n", what);
        if (!told) { describe(list, n, source, P); told = true; }
    }
};

// a value: the hash of an op, its entry and its inputs; 0 is "nothing written yet"
static uint64_t mix(uint64_t op, uint64_t entry, uint64_t a, uint64_t b) {
    uint64_t h = 0x9e3779b97f4a7c15ull ^ (op * 0xff51afd7ed558ccdull) ^ (entry << 56);
    for (uint64_t v : {a, b}) { h ^= v + 0x9e3779b97f4a7c15ull + (h << 6) + (h >> 2); h *= 0xc4ceb9fe1a85ec53ull; h ^= h >> 33; }
    return h | 1u;
}
static const uint64_t GROUP = 0x1234567u;
static uint64_t value_of(Op op, uint32_t entry, uint64_t src, uint64_t group) { return mix(uint64_t(op) + 1, entry, src, op == Op::SHADOW_FINISH ? group : 0); }

// the sequential model, pass by pass: what every launch of the list writes, in order
static std::vector<uint64_t> model(const swfr_filter* list, uint32_t n, Source source, uint32_t* boxes, uint32_t* shadows, uint32_t* convs) {
    std::vector<uint64_t> out;
    uint64_t r = GROUP;
    *boxes = *shadows = *convs = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const swfr_shadow& S = list[i].shadow;
        const auto box_passes = [&](uint64_t v) {
            for (uint32_t p = 0; p < S.passes; ++p) {
                if (S.blur_x > 1u) { v = value_of(Op::BOX_H, i, v, 0); out.push_back(v); ++*boxes; }
                if (S.blur_y > 1u) { v = value_of(Op::BOX_V, i, v, 0); out.push_back(v); ++*boxes; }
            }
            return v;
        };
        if (list[i].kind == SWFR_FILTER_CONVOLUTION) {
            r = value_of(Op::CONVOLVE, i, r, 0); out.push_back(r); ++*convs;
        } else if (list[i].kind == SWFR_FILTER_SHADOW) {
            uint64_t a = value_of(Op::SHADOW_ALPHA, i, r, 0); out.push_back(a);
            a = box_passes(a);
            r = value_of(Op::SHADOW_FINISH, i, a, r); out.push_back(r); ++*shadows;
        } else {
            if (i == 0 && source == Source::Framebuffer) { r = value_of(Op::CAPTURE, i, r, 0); out.push_back(r); }   // framebuffer words to texels
            r = box_passes(r);
        }
    }
    return out;
}

static void one(const swfr_filter* list, uint32_t n, Source source) {
    const FilterPlan P = plan_filters(list, n, source);
    Checker check{list, n, source, P};
    uint32_t boxes, shadows, convs;
    const std::vector<uint64_t> want = model(list, n, source, &boxes, &shadows, &convs);
    const bool fb = source == Source::Framebuffer;
    uint64_t held[4] = {fb ? GROUP : 0, fb ? 0 : GROUP, 0, 0};
    bool named[4] = {false, false, false, false};
    uint32_t passes = 0, copies = 0;
    check(P.n <= MAX_FILTER_STEPS, "the plan fits its bound");
    for (uint32_t k = 0; k < P.n && k < MAX_FILTER_STEPS; ++k) {
        const FilterStep& s = P.steps[k];
        const bool finish = s.op == Op::SHADOW_FINISH;
        check(s.src <= T2 && s.dst <= T2 && s.group <= T2 && s.entry < n, "a step names a buffer and an entry of the list");
        if (s.src > T2 || s.dst > T2 || s.group > T2 || s.entry >= n) return;
        named[s.src] = named[s.dst] = true;
        if (finish) named[s.group] = true;
        check(finish || s.group == s.src, "only a finish pass has a group of its own");
        check(s.dst != FB, "the framebuffer is never a destination");
        check(s.src != s.dst || finish, "only a finish pass runs in place");
        check(held[s.src] != 0 && (!finish || held[s.group] != 0), "a step reads what an earlier step wrote");
        if (s.op == Op::COPY) {
            ++copies;
            check(k + 1 == P.n && !fb, "a copy is the last step of a texel plan");
            check(s.src == T1 && s.dst == T0, "the copy brings the result from T1 to T0");
            held[s.dst] = held[s.src];
            continue;
        }
        const uint64_t v = value_of(s.op, s.entry, held[s.src], held[s.group]);
        // (a step that read a buffer overwritten since with another value writes another value than the model's pass)
        check(passes < want.size() && v == want[passes], "the k-th pass writes what the model's k-th pass writes: every value it read was still live");
        ++passes;
        held[s.dst] = v;
    }
    check(passes == want.size(), "as many passes as the sequential model runs");
    check(held[T0] == (want.empty() ? (fb ? 0 : GROUP) : want.back()), "T0 ends holding f_n(... f_1(group))");
    check(held[FB] == (fb ? GROUP : 0), "the framebuffer is as it was");
    for (int b = FB; b <= T2; ++b) check(P.uses[b] == named[b], "uses[] is true exactly for the buffers the steps name");
    const uint32_t capture = fb && list[0].kind == SWFR_FILTER_BLUR ? 1u : 0u;
    check(P.n - copies == boxes + 2 * shadows + convs + capture, "box steps + 2 per shadow + 1 per convolution (+ the capture of a first blur)");
    check(copies <= (fb ? 0u : 1u), "no copy from the framebuffer, at most one from texels");
}

static const uint32_t N_TYPES = 25;
static swfr_filter entry_type(uint32_t t) {
    swfr_filter F{};
    if (t == 24) { F.kind = SWFR_FILTER_CONVOLUTION; F.shadow.blur_x = 7; return F; }     // (blur_x: the kernel slot)
    const uint32_t j = t % 12;
    F.kind = t < 12 ? SWFR_FILTER_BLUR : SWFR_FILTER_SHADOW;
    F.shadow.blur_x = (j & 1u) ? 3 : 1; F.shadow.blur_y = (j & 2u) ? 4 : 0; F.shadow.passes = 1 + j / 4;
    if (t >= 12) { F.shadow.dx = 3; F.shadow.dy = -2; F.shadow.color = swfr_rgba8{10, 20, 30, 200}; F.shadow.strength = 2; F.shadow.flags = (j & 1u) ? SWFR_SHADOW_INNER : 0u; }
    return F;
}
static bool is(const FilterStep& s, Op op, Buffer src, Buffer dst) { return s.op == op && s.src == src && s.dst == dst; }

int main() {
    static_assert(SWFR_MAX_FILTERS == 4, "the enumeration below nests four loops");
    static_assert(MAX_FILTER_STEPS == SWFR_MAX_FILTERS * (2 * 15 + 2) + 1, "the step bound");
    unsigned long lists = 0;
    uint32_t box_counts = 0;
    for (uint32_t t = 0; t < 12; ++t) { const swfr_filter F = entry_type(t); box_counts |= 1u << blur_steps(F.shadow.blur_x, F.shadow.blur_y, F.shadow.passes); }
    if (box_counts != 0x5fu) { ++failures; std::printf("FAIL the blurs have 0, 1, 2, 3, 4 and 6 box steps (mask %x)\n", box_counts); }
    for (Source source : {Source::Framebuffer, Source::Texels}) {
        swfr_filter list[SWFR_MAX_FILTERS];
        for (uint32_t a = 0; a < N_TYPES; ++a) {
            list[0] = entry_type(a); one(list, 1, source); ++lists;
            for (uint32_t b = 0; b < N_TYPES; ++b) {
                list[1] = entry_type(b); one(list, 2, source); ++lists;
                for (uint32_t c = 0; c < N_TYPES; ++c) {
                    list[2] = entry_type(c); one(list, 3, source); ++lists;
                    for (uint32_t d = 0; d < N_TYPES; ++d) { list[3] = entry_type(d); one(list, 4, source); ++lists; }
                }
            }
        }
    }
    // the longest plans there are (15 passes, both axes): inside the bound, and inside the array (ASan)
    {
        swfr_filter list[SWFR_MAX_FILTERS];
        for (uint32_t i = 0; i < SWFR_MAX_FILTERS; ++i) { list[i] = entry_type(12); list[i].shadow.blur_x = 255; list[i].shadow.blur_y = 255; list[i].shadow.passes = 15; }
        for (Source source : {Source::Framebuffer, Source::Texels}) {
            one(list, SWFR_MAX_FILTERS, source);
            const FilterPlan P = plan_filters(list, SWFR_MAX_FILTERS, source);
            if (P.n != SWFR_MAX_FILTERS * 32) { ++failures; std::printf("FAIL four shadows of 15 passes are %u steps\n", P.n); }
        }
        list[SWFR_MAX_FILTERS - 1] = entry_type(24);
        one(list, SWFR_MAX_FILTERS, Source::Framebuffer);
        one(list, SWFR_MAX_FILTERS, Source::Texels);
        if (plan_filters(list, SWFR_MAX_FILTERS, Source::Texels).n != (SWFR_MAX_FILTERS - 1) * 32 + 2) { ++failures; std::printf("FAIL three long shadows, a convolution and the copy\n"); }
    }
    // the special cases by name
    {
        const swfr_filter box1 = entry_type(0), conv = entry_type(24);
        FilterPlan P = plan_filters(&box1, 1, Source::Framebuffer);
        if (!(P.n == 1 && is(P.steps[0], Op::CAPTURE, FB, T0) && P.uses[T0] && !P.uses[T1] && !P.uses[T2])) { ++failures; std::printf("FAIL a lone 1 x 1 blur of the framebuffer is one capture into T0\n"); }
        P = plan_filters(&conv, 1, Source::Framebuffer);
        if (!(P.n == 1 && is(P.steps[0], Op::CONVOLVE, FB, T0) && !P.uses[T1] && !P.uses[T2])) { ++failures; std::printf("FAIL a lone convolution of the framebuffer goes straight into T0\n"); }
        P = plan_filters(&conv, 1, Source::Texels);
        if (!(P.n == 2 && is(P.steps[0], Op::CONVOLVE, T0, T1) && is(P.steps[1], Op::COPY, T1, T0))) { ++failures; std::printf("FAIL a lone convolution of texels goes to T1 and is copied back\n"); }
        P = plan_filters(&box1, 1, Source::Texels);
        if (!(P.n == 0 && !P.uses[FB] && !P.uses[T0] && !P.uses[T1] && !P.uses[T2])) { ++failures; std::printf("FAIL a 1 x 1 blur of texels is no step at all\n"); }
    }
    if (failures) { std::printf("%d checks failed\n", failures); return 1; }
    std::printf("filter plans ok: %lu lists\n", lists);
    return 0;
}
"""


def _build_and_run(tmp_path, name, extra):
    gxx = shutil.which("g++")
    assert gxx, "the host g++ is needed to check filter_plan.hpp"
    src = tmp_path / "filter_plan_check.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / name
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I" + CSRC] + extra + [str(src), "-o", str(exe)])
    run = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0 and "filter plans ok: 813800 lists" in run.stdout, run.stdout


def test_every_plan_computes_the_sequential_model(tmp_path):
    _build_and_run(tmp_path, "check", [])


def test_the_planner_runs_clean_under_asan_and_ubsan(tmp_path):
    """The same stand-alone program (nothing loaded into Python) with the sanitizers: the longest plans fill the step array."""
    _build_and_run(tmp_path, "check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
