// filter_plan.hpp -- a filter list as an ordered list of passes over four buffers.  Host code only, no HIP: renderer.cpp runs a plan
// (run_filter_plan), tests/test_filter_plan.py enumerates the lists and interprets every plan without a device.
//
// The planner's contract.  Four buffers of one size take part:
//   FB  the sub-frame's framebuffer: RGBA words, read only, never a destination
//   T0  the layer texture, or a bitmap's own texels: where every plan leaves its result
//   T1  blur_scratch
//   T2  shadow_scratch: the alpha surface of a shadow behind another entry, and nothing else
// Source::Framebuffer (a filtered layer of swfr_render): the group lies in FB.  The first entry reads it: a blur through one CAPTURE,
// a shadow through its alpha pass and, behind its box passes, its finish pass in place over the blurred alpha with FB as the group, a
// convolution straight into the buffer it must end in (no capture in front of it).  Source::Texels (swfr_blur_bitmap,
// swfr_convolve_bitmap): the group lies in T0 as ARGB texels, and the first entry is planned as every later one.
// Every later entry reads the result before it as ARGB texels, from T0 or T1.  A blur's box passes alternate between that buffer and
// the other of the two; a convolution is one out-of-place step to the other of the two.  A shadow keeps its group where it is: its
// alpha pass goes to the other of T0 and T1, its box passes alternate between that and T2, and its finish pass runs in place over the
// group.  So an entry ends where it began, or -- a convolution, a blur of an odd number of box steps -- in the other of T0 and T1.
// Those parities, summed over the later entries, say where the first entry of a framebuffer plan must end for the last one to end in
// T0, and so where it puts its capture or alpha pass: a framebuffer plan has no COPY.  A texel plan begins in T0 and has one trailing
// COPY from T1 to T0 when the parities leave the result there.  Nothing waits between steps: they run in order on one stream.
#pragma once
#include <stdint.h>

#include "../../include/swfr.h"

namespace swfr {

enum Buffer : uint8_t { FB = 0, T0 = 1, T1 = 2, T2 = 3 };
enum class Op : uint8_t { CAPTURE, BOX_H, BOX_V, SHADOW_ALPHA, SHADOW_FINISH, CONVOLVE, COPY };
enum class Source : uint8_t { Framebuffer, Texels };

// One pass: `op` reads src and writes dst.  SHADOW_FINISH reads the blurred alpha at src and the group surface at `group` (FB or a
// texture; dst may be either of the two: the pass is pointwise); every other op leaves group == src.  `entry` indexes the filter list:
// the executor takes box widths, offsets, colour, strength, flags and the kernel from there (COPY: the last entry, unused).
struct FilterStep { Op op; Buffer src, dst, group; uint8_t entry; };

constexpr uint32_t MAX_FILTER_STEPS = SWFR_MAX_FILTERS * (2 * 15 + 2) + 1;   // per entry 15 passes of two boxes, alpha and finish; one COPY

struct FilterPlan {
    uint32_t n = 0;
    FilterStep steps[MAX_FILTER_STEPS];
    bool uses[4] = {false, false, false, false};      // the buffers the steps name: what a caller has to have reserved
};

// the box passes of a blur that do something: a width of 0 or 1 leaves its axis alone
inline uint32_t blur_steps(uint32_t blur_x, uint32_t blur_y, uint32_t passes) { return passes * ((blur_x > 1u ? 1u : 0u) + (blur_y > 1u ? 1u : 0u)); }

inline FilterPlan plan_filters(const swfr_filter* list, uint32_t n, Source source) {
    FilterPlan P;
    const auto other = [](Buffer b) { return b == T0 ? T1 : T0; };
    const auto emit = [&P](Op op, Buffer src, Buffer dst, Buffer group, uint32_t entry) {
        P.steps[P.n++] = FilterStep{op, src, dst, group, uint8_t(entry)};
        P.uses[src] = P.uses[dst] = P.uses[group] = true;
    };
    // entry i's box passes over the image at `a`, alternating with `b`: returns where the result lies
    const auto boxes = [&](uint32_t i, Buffer a, Buffer b) {
        const swfr_shadow& S = list[i].shadow;
        for (uint32_t p = 0; p < S.passes; ++p)
            for (int vertical = 0; vertical < 2; ++vertical) {
                if ((vertical ? S.blur_y : S.blur_x) <= 1u) continue;
                emit(vertical ? Op::BOX_V : Op::BOX_H, a, b, a, i);
                const Buffer t = a; a = b; b = t;
            }
        return a;
    };
    // whether entry i, reading texels, ends in the other of T0 and T1
    const auto flips = [&](uint32_t i) {
        const swfr_filter& F = list[i];
        if (F.kind == SWFR_FILTER_CONVOLUTION) return true;
        return F.kind != SWFR_FILTER_SHADOW && (blur_steps(F.shadow.blur_x, F.shadow.blur_y, F.shadow.passes) & 1u) != 0u;
    };
    Buffer at = T0;                                   // where the result so far lies
    uint32_t i = 0;
    if (source == Source::Framebuffer && n) {
        for (uint32_t k = 1; k < n; ++k) if (flips(k)) at = other(at);     // where the first entry must end
        const swfr_filter& F = list[0];
        if (F.kind == SWFR_FILTER_CONVOLUTION) {
            emit(Op::CONVOLVE, FB, at, FB, 0);
        } else {
            const bool odd = (blur_steps(F.shadow.blur_x, F.shadow.blur_y, F.shadow.passes) & 1u) != 0u;
            const Buffer first = odd ? other(at) : at;
            emit(F.kind == SWFR_FILTER_SHADOW ? Op::SHADOW_ALPHA : Op::CAPTURE, FB, first, FB, 0);
            boxes(0, first, other(first));
            if (F.kind == SWFR_FILTER_SHADOW) emit(Op::SHADOW_FINISH, at, at, FB, 0);
        }
        i = 1;
    }
    for (; i < n; ++i) {
        const swfr_filter& F = list[i];
        if (F.kind == SWFR_FILTER_CONVOLUTION) {
            emit(Op::CONVOLVE, at, other(at), at, i);
            at = other(at);
        } else if (F.kind == SWFR_FILTER_SHADOW) {
            emit(Op::SHADOW_ALPHA, at, other(at), at, i);
            const Buffer alpha = boxes(i, other(at), T2);
            emit(Op::SHADOW_FINISH, alpha, at, at, i);
        } else {
            at = boxes(i, at, other(at));
        }
    }
    if (at != T0) emit(Op::COPY, T1, T0, T1, n - 1);  // (a texel plan only: a framebuffer plan was begun so as to end in T0)
    return P;
}

}  // namespace swfr
