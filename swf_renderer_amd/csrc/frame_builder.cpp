// frame_builder.cpp -- see frame_builder.hpp.
#include "frame_builder.hpp"

#include <atomic>
#include <chrono>
#include <cstdlib>
#include <functional>

#include <algorithm>
#include <cstring>

namespace swfr {
namespace {

inline double lerp(double a, double b, double r) { return b * r + a * (1 - r); }  // canvas-renderer.ts:24-26

struct Css {
    int r, g, b, a;
};
// fromNormalizedColor (ts/src/lib/css-color.ts:11-13) then node-canvas' CSS colour parse: R is
// `& 0xff`-truncated, G/B truncate to ints, alpha is quantised to 8 bits in float.
Css css_color(double r, double g, double b, double a) {
    Css c;
    c.r = int(r * 255.0) & 0xff;
    c.g = std::clamp(int(g * 255.0), 0, 255);
    c.b = std::clamp(int(b * 255.0), 0, 255);
    const float af = float(std::clamp(a, 0.0, 1.0));
    c.a = int(af * 255.0f);
    return c;
}
// cairo_set_source_rgba(r/255, g/255, b/255, a/255): premultiply in doubles, 16-bit shorts, >> 8.
uint32_t premultiplied_pixel(const Css& c) {
    const double r = c.r / 255.0, g = c.g / 255.0, b = c.b / 255.0, a = c.a / 255.0;
    auto sh = [](double v) { return uint32_t(uint16_t(v * 65535.0 + 0.5)) >> 8; };
    return (sh(a) << 24) | (sh(r * a) << 16) | (sh(g * a) << 8) | sh(b * a);
}
Css morph_color(const swfr_rgba8& s, const swfr_rgba8& e, bool morph, double ratio) {
    if (!morph) return css_color(s.r / 255.0, s.g / 255.0, s.b / 255.0, s.a / 255.0);
    return css_color(lerp(s.r / 255.0, e.r / 255.0, ratio), lerp(s.g / 255.0, e.g / 255.0, ratio),
                     lerp(s.b / 255.0, e.b / 255.0, ratio), lerp(s.a / 255.0, e.a / 255.0, ratio));
}

// SWF blend-mode number -> path operator ("Blend modes"): the eight modes Cairo has an operator for; the others need an
// isolated group (layer, alpha, erase) or have no Cairo operator (subtract, invert)
// (SWFR_FLAG_ALPHA_MODES: erase is DEST_OUT, per path too; alpha -- DEST_IN, unbounded -- is a layer's mode only: layer_operator)
uint32_t blend_operator(uint32_t mode, bool alpha_modes) {
    if (alpha_modes && mode == SWFR_BLEND_ERASE) return SWFR_OP_ERASE;
    switch (mode) {
        case SWFR_BLEND_NORMAL0: case SWFR_BLEND_NORMAL: return SWFR_OP_OVER;
        case SWFR_BLEND_MULTIPLY: return SWFR_OP_MULTIPLY;
        case SWFR_BLEND_SCREEN: return SWFR_OP_SCREEN;
        case SWFR_BLEND_LIGHTEN: return SWFR_OP_LIGHTEN;
        case SWFR_BLEND_DARKEN: return SWFR_OP_DARKEN;
        case SWFR_BLEND_DIFFERENCE: return SWFR_OP_DIFFERENCE;
        case SWFR_BLEND_ADD: return SWFR_OP_ADD;
        case SWFR_BLEND_OVERLAY: return SWFR_OP_OVERLAY;
        case SWFR_BLEND_HARDLIGHT: return SWFR_OP_HARDLIGHT;
        default: break;
    }
    if (mode <= SWFR_BLEND_HARDLIGHT) throw StatusError{SWFR_ERR_NOT_IMPLEMENTED, "NotImplementedBlendMode"};
    throw StatusError{SWFR_ERR_INVALID, "InvalidBlendMode"};
}
// the operator an isolated layer (SWFR_OBJECT_LAYER) is composited with: OVER also for "layer", the mode whose whole meaning is the group
uint32_t layer_operator(uint32_t mode, bool alpha_modes) {
    if (alpha_modes && mode == SWFR_BLEND_ALPHA) return SWFR_OP_ALPHA;
    return mode == SWFR_BLEND_LAYER ? uint32_t(SWFR_OP_OVER) : blend_operator(mode, alpha_modes);
}
// a path's blend field once it is known whether the surface was still clear when it was drawn: "2" (a lerp only because nothing was
// painted yet -- an OVER or an ADD path) becomes the SOURCE lerp, or what the path is otherwise: OVER, or its operator
inline uint32_t settle_lerp(uint32_t lerp, bool clear) { return (lerp & 0xffu) == 2u ? (clear ? 1u : (lerp & ~0xffu)) : lerp; }

// a worker builder met a blurred layer: sub-frames are built by one walk only, so build() walks the stage again on its own (never
// leaves the builder)
constexpr int BLUR_IN_PIECE = -16;

}  // namespace

bool shadow_valid(const swfr_shadow& s) {
    return s.blur_x <= 255u && s.blur_y <= 255u && s.passes >= 1u && s.passes <= 15u && s.dx >= -32768 && s.dx <= 32767 && s.dy >= -32768 &&
           s.dy <= 32767 && s.strength >= 1u && s.strength <= 255u &&
           (s.flags <= SWFR_SHADOW_KNOCKOUT || s.flags == SWFR_SHADOW_INNER || s.flags == (SWFR_SHADOW_INNER | SWFR_SHADOW_KNOCKOUT));   // 0, 1, 2, 8, 10
}
uint32_t shadow_color_pixel(const swfr_rgba8& c) { return premultiplied_pixel(Css{c.r, c.g, c.b, c.a}); }
bool filter_valid(const swfr_filter& f) {
    if (f.kind == SWFR_FILTER_SHADOW) return shadow_valid(f.shadow);
    const swfr_shadow& s = f.shadow;
    const bool rest_zero = s.dx == 0 && s.dy == 0 && s.color.r == 0 && s.color.g == 0 && s.color.b == 0 && s.color.a == 0 && s.strength == 0u && s.flags == 0u;
    if (f.kind == SWFR_FILTER_CONVOLUTION) return s.blur_x <= 65535u && s.blur_y == 0u && s.passes == 0u && rest_zero;   // (blur_x: the kernel slot)
    if (f.kind != SWFR_FILTER_BLUR) return false;
    return s.blur_x <= 255u && s.blur_y <= 255u && s.passes >= 1u && s.passes <= 15u && rest_zero;
}
bool kernel_valid(const swfr_kernel& k) {
    if (k.width < 1u || k.width > SWFR_MAX_KERNEL_DIM || k.height < 1u || k.height > SWFR_MAX_KERNEL_DIM) return false;
    int64_t sum = 0;
    for (uint32_t i = 0; i < k.width * k.height; ++i) sum += k.taps[i] < 0 ? -int64_t(k.taps[i]) : int64_t(k.taps[i]);
    return sum <= 8388607;
}

bool color_transform_valid(const swfr_color_transform& ct) {
    for (int k = 0; k < 4; ++k)
        if (ct.mult[k] < INT16_MIN || ct.mult[k] > INT16_MAX || ct.add[k] < INT16_MIN || ct.add[k] > INT16_MAX) return false;
    return true;
}

swfr_rgba8 FrameBuilder::cx(const swfr_rgba8& c) const {
    const int32_t li = stack_.back().lut;
    if (li < 0) return c;
    const ColorLut& L = luts_[size_t(li)];
    return swfr_rgba8{L.t[0][c.r], L.t[1][c.g], L.t[2][c.b], L.t[3][c.a]};
}

// c' = clamp(((c * mult) >> 8) + add, 0, 255) per channel (int32, arithmetic shift), then the outer chain: nested transforms apply
// innermost first and each one clamps, so a chain is a table per channel and nothing less.  Chains are kept once per content and
// an all-identity chain is -1, so that an identity wrapper changes nothing at all.
int32_t FrameBuilder::compose(int32_t outer, const swfr_color_transform& inner) {
    const auto memo_key = std::make_pair(outer, std::string(reinterpret_cast<const char*>(&inner), sizeof inner));
    const auto hit = compose_memo_.find(memo_key);
    if (hit != compose_memo_.end()) return hit->second;
    ColorLut L;
    bool identity = true;
    for (int ch = 0; ch < 4; ++ch)
        for (int c = 0; c < 256; ++c) {
            const int32_t v = std::clamp(((c * inner.mult[ch]) >> 8) + inner.add[ch], 0, 255);
            const uint8_t out = outer < 0 ? uint8_t(v) : luts_[size_t(outer)].t[ch][v];
            L.t[ch][c] = out;
            identity = identity && out == c;
        }
    int32_t index = -1;
    if (!identity) {
        std::string bytes(reinterpret_cast<const char*>(&L), sizeof L);
        const auto it = lut_index_.find(bytes);
        if (it != lut_index_.end()) index = it->second;
        else {
            index = int32_t(luts_.size());
            luts_.push_back(L);
            lut_index_.emplace(std::move(bytes), index);
        }
    }
    compose_memo_.emplace(memo_key, index);
    return index;
}

uint32_t FrameBuilder::variant_of(uint32_t bitmap, int32_t lut) {
    const auto key = std::make_pair(bitmap, lut);
    const auto it = variant_index_.find(key);
    if (it != variant_index_.end()) return it->second;
    const uint32_t k = uint32_t(variants_.size());
    variants_.push_back(TextureVariant{bitmap, luts_[size_t(lut)]});
    variant_index_.emplace(key, k);
    return k;
}

Affine FrameBuilder::matrix_of(const swfr_matrix& m) {
    // applyMatrix (canvas-renderer.ts:179-188): transform(scaleX, rotateSkew0, rotateSkew1, scaleY, tx, ty)
    Affine a;
    a.xx = m.scale_x / 65536.0;
    a.yx = m.rotate_skew0 / 65536.0;
    a.xy = m.rotate_skew1 / 65536.0;
    a.yy = m.scale_y / 65536.0;
    a.x0 = m.translate_x;
    a.y0 = m.translate_y;
    return a;
}

const DecodedShape* FrameBuilder::shape(uint32_t id, bool morph) const {
    const auto& v = morph ? store()->morphs_ : store()->shapes_;
    return id < v.size() ? &v[id] : nullptr;
}

// ---- worker threads: a fixed set, woken per frame (generation counter), each running one job index of the current task
struct FrameBuilder::Pool {
    std::vector<std::thread> threads;                          // thread i (1-based) runs job i of a task when the task has that many jobs
    std::vector<std::unique_ptr<FrameBuilder>> builders;       // one builder per piece
    std::mutex m;
    std::condition_variable cv_go, cv_done;
    std::atomic<uint64_t> generation{0};
    std::atomic<int> pending{0};
    std::atomic<bool> quit{false};
    int n_jobs = 0;
    std::function<void(int)> task;
    // Frames arrive a few hundred microseconds apart while an animation is rendered: a worker that has just finished keeps polling for
    // that long before it blocks (a sleeping core takes longer to wake than a piece takes to build), and the caller polls for the
    // pieces' completion likewise.
    static constexpr long SPIN_NS = 400000;
    static long now_ns() { return std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
    static void relax() {
#if defined(__x86_64__) || defined(__i386__)
        __builtin_ia32_pause();
#endif
    }
    void run(int jobs, std::function<void(int)> fn) {           // jobs 1 .. jobs-1 on the pool, job 0 here; returns when all are done
        task = std::move(fn);
        n_jobs = jobs;
        // every worker takes part in every generation (one without a job only counts itself off): run() cannot return -- and the next
        // run() cannot rewrite task / n_jobs -- while a worker is still between noticing the generation and reading them
        pending.store(int(threads.size()), std::memory_order_relaxed);
        generation.fetch_add(1, std::memory_order_release);    // (publishes task / n_jobs / pending)
        { std::lock_guard<std::mutex> lk(m); }                  // a worker between its predicate check and its wait sees the new generation or gets the notification
        cv_go.notify_all();
        task(0);
        const long t0 = now_ns();
        while (pending.load(std::memory_order_acquire) != 0) {
            if (now_ns() - t0 > SPIN_NS) {
                std::unique_lock<std::mutex> lk(m);
                cv_done.wait(lk, [&] { return pending.load(std::memory_order_acquire) == 0; });
                break;
            }
            relax();
        }
    }
    void worker(int index) {
        uint64_t seen = 0;
        for (;;) {
            const long t0 = now_ns();
            uint64_t g;
            while ((g = generation.load(std::memory_order_acquire)) == seen && !quit.load(std::memory_order_relaxed)) {
                if (now_ns() - t0 > SPIN_NS) {
                    std::unique_lock<std::mutex> lk(m);
                    cv_go.wait(lk, [&] { return quit.load() || generation.load(std::memory_order_acquire) != seen; });
                } else relax();
            }
            if (quit.load()) return;
            seen = g;
            if (index < n_jobs) task(index);                    // (a task with fewer jobs: nothing to do but to count off)
            if (pending.fetch_sub(1, std::memory_order_acq_rel) == 1) {
                { std::lock_guard<std::mutex> lk(m); }
                cv_done.notify_one();
            }
        }
    }
};

FrameBuilder::FrameBuilder(uint32_t width, uint32_t height, bool even_odd, bool aliased, bool linear_pixman, bool alpha_modes)
    : w_(width), h_(height), even_odd_(even_odd), aliased_(aliased), linear_pixman_(linear_pixman), alpha_modes_(alpha_modes) {}

FrameBuilder::~FrameBuilder() {
    if (pool_) {
        pool_->quit.store(true);
        { std::lock_guard<std::mutex> lk(pool_->m); }
        pool_->cv_go.notify_all();
        for (auto& t : pool_->threads) t.join();
    }
}

void FrameBuilder::build_range(const std::vector<const swfr_display_object*>& wraps, const swfr_display_object* kids, uint32_t lo, uint32_t hi) {
    edges_.clear();
    paths_.clear();
    styles_.clear();
    stack_.clear();
    luts_.clear(); lut_index_.clear(); compose_memo_.clear(); variant_index_.clear(); variants_.clear();
    failed_ = false;
    group_depth_ = 0;
    layers_.clear();
    in_blur_ = false;
    surface_clear_ = true;  // clearRect over the whole canvas (canvas-renderer.ts:70-71); a later piece learns the truth when joined
    drawn_ = PixelRect{};
    State s;
    s.ctm = Affine::scale(1.0 / 20.0, 1.0 / 20.0);  // twips -> px (:74)
    s.inv = Affine::scale(1.0 / (1.0 / 20.0), 1.0 / (1.0 / 20.0));  // cairo_scale: ctm_inverse *= scale(1/sx, 1/sy)
    stack_.push_back(s);
    try {
        // the wrappers the children sit in (see build): their matrices and colour transforms, as draw() applies them
        for (const swfr_display_object* w : wraps) {
            stack_.push_back(stack_.back());
            if (w->has_matrix) transform(matrix_of(w->matrix));
            if (w->type == SWFR_OBJECT_COLOR_TRANSFORM) {
                const auto it = store()->cxforms_.find(w->id);
                if (it == store()->cxforms_.end()) throw StatusError{SWFR_ERR_NOT_FOUND, "ColorTransformNotFound"};
                stack_.back().lut = compose(stack_.back().lut, it->second);
            }
            if (w->type == SWFR_OBJECT_BLEND_MODE) stack_.back().op = blend_operator(w->id, alpha_modes_);
        }
        for (uint32_t i = lo; i < hi; ++i) draw(kids[i], int(wraps.size()));
    } catch (const StatusError& e) {
        failed_ = true;
        failure_ = e;
    }
}

// this piece's arrays into their place in the joined frame: indices shifted, the "still clear?" lerps settled
void FrameBuilder::copy_piece(FrameBuilder& dst, size_t edge_off, size_t path_off, size_t style_off, bool clear_at_start,
                              const std::vector<uint32_t>& variant_map) const {
    for (size_t i = 0; i < edges_.size(); ++i) {
        swfr_edge e = edges_[i];
        e.reserved += int32_t(path_off);
        dst.edges_[edge_off + i] = e;
    }
    for (size_t i = 0; i < paths_.size(); ++i) {
        swfr_path p = paths_[i];
        p.first_edge += uint32_t(edge_off);
        if (p.kind < SWFR_PATH_GROUP_BEGIN) p.style += uint32_t(style_off);      // (a group marker has no style: its field stays 0)
        p.lerp = settle_lerp(p.lerp, clear_at_start);           // (inside the piece the flag is only ever 2 while nothing was painted)
        dst.paths_[path_off + i] = p;
    }
    if (!styles_.empty()) std::memcpy(&dst.styles_[style_off], styles_.data(), styles_.size() * sizeof(swfr_style));
    if (!variants_.empty())                                     // the piece's textures renumbered to the joined frame's
        for (size_t i = 0; i < styles_.size(); ++i) {
            swfr_style& st = dst.styles_[style_off + i];
            if (st.kind == SWFR_STYLE_BITMAP && st.bitmap >= VARIANT_BASE) st.bitmap = VARIANT_BASE + variant_map[st.bitmap - VARIANT_BASE];
        }
}

void FrameBuilder::build(const swfr_stage& stage) {
    layers_.clear();          // (a build in pieces never runs build_range on this builder: the last frame's sub-frames go here)
    in_blur_ = false;
    int want = threads_;
    if (want < 0) {
        const char* env = std::getenv("SWFR_BUILD_THREADS");
        want = env ? std::atoi(env) : int(std::min(8u, std::max(1u, std::thread::hardware_concurrency())));
        threads_ = want;
    }
    // The objects that are cut into pieces: the stage's children -- or, when the stage holds one container, colour-transform or
    // blend-mode wrapper (a whole clip under one fade), that wrapper's children, through up to 16 such single wrappers.  A piece then walks its share of them
    // inside the wrappers' state, which is what a single walk does: the wrappers draw nothing themselves.
    std::vector<const swfr_display_object*> wraps;
    const swfr_display_object* kids = stage.children;
    uint32_t n_kids = stage.n_children;
    while (n_kids == 1 && wraps.size() < 16 && (kids[0].type == SWFR_OBJECT_CONTAINER || kids[0].type == SWFR_OBJECT_COLOR_TRANSFORM || kids[0].type == SWFR_OBJECT_BLEND_MODE)) {
        wraps.push_back(&kids[0]);
        n_kids = kids[0].n_children;
        kids = kids[0].children;
    }
    // pieces of at least 64 display objects each.  (SWFR_FLAG_ALPHA_MODES: one walk -- an ALPHA layer's rectangle takes in every path
    // drawn on its surface before it, which a piece does not know of the pieces before it)
    const int pieces = alpha_modes_ ? 1 : int(std::min<uint32_t>(uint32_t(std::max(want, 1)), n_kids / 64));
    if (pieces < 2) {
        build_range({}, stage.children, 0, stage.n_children);
        if (failed_) throw failure_;
        for (swfr_path& p : paths_) p.lerp = settle_lerp(p.lerp, true);
        return;
    }
    if (!pool_) pool_.reset(new Pool);
    Pool& P = *pool_;
    while (int(P.builders.size()) < pieces) {                 // (piece k is built by builders[k-1] for k >= 1; piece 0 needs a scratch builder, too)
        P.builders.emplace_back(new FrameBuilder(w_, h_, even_odd_, aliased_, linear_pixman_, alpha_modes_));
        P.builders.back()->parent_ = this;
        P.builders.back()->threads_ = 0;
    }
    while (int(P.threads.size()) < pieces - 1) {
        const int index = int(P.threads.size()) + 1;
        P.threads.emplace_back([&P, index] { P.worker(index); });
    }
    auto lo_of = [&](int k) { return uint32_t(uint64_t(n_kids) * uint64_t(k) / uint64_t(pieces)); };
    // ---- phase A: every piece into its own builder
    P.run(pieces, [&](int k) { P.builders[k]->build_range(wraps, kids, lo_of(k), lo_of(k + 1)); });
    for (int k = 0; k < pieces; ++k)
        if (P.builders[k]->failed_ && P.builders[k]->failure_.code == BLUR_IN_PIECE) {
            // a frame with a blurred layer: one walk, which keeps the layers' sub-frames and numbers them in painter's order
            build_range({}, stage.children, 0, stage.n_children);
            if (failed_) throw failure_;
            for (swfr_path& p : paths_) p.lerp = settle_lerp(p.lerp, true);
            return;
        }
    size_t ne = 0, np = 0, ns = 0;
    std::vector<size_t> eo(pieces), po(pieces), so(pieces);
    std::vector<char> clear_at(pieces);
    bool clear = true;
    for (int k = 0; k < pieces; ++k) {
        const FrameBuilder& B = *P.builders[k];
        if (B.failed_) throw B.failure_;                      // the first failing display object in painter's order, as a single walk would report
        eo[k] = ne; po[k] = np; so[k] = ns; clear_at[k] = clear;
        ne += B.edges_.size(); np += B.paths_.size(); ns += B.styles_.size();
        clear = clear && B.surface_clear_;
    }
    edges_.resize(ne); paths_.resize(np); styles_.resize(ns);
    surface_clear_ = clear;
    // the pieces' texture variants in painter's order, each (bitmap, chain) once: the numbering a single walk gives them
    variants_.clear();
    std::vector<std::vector<uint32_t>> vmap(pieces);
    {
        std::map<std::pair<uint32_t, std::string>, uint32_t> seen;
        for (int k = 0; k < pieces; ++k)
            for (const TextureVariant& v : P.builders[k]->variants_) {
                auto key = std::make_pair(v.bitmap, std::string(reinterpret_cast<const char*>(&v.lut), sizeof v.lut));
                auto it = seen.find(key);
                if (it == seen.end()) {
                    it = seen.emplace(std::move(key), uint32_t(variants_.size())).first;
                    variants_.push_back(v);
                }
                vmap[k].push_back(it->second);
            }
    }
    // ---- phase B: the pieces copied to their places, in parallel
    P.run(pieces, [&](int k) { P.builders[k]->copy_piece(*this, eo[k], po[k], so[k], clear_at[k] != 0, vmap[k]); });
}

void FrameBuilder::draw(const swfr_display_object& obj, int depth) {
    if (depth > 256) throw StatusError{SWFR_ERR_INVALID, "display tree too deep"};
    stack_.push_back(stack_.back());  // context.save()
    struct Pop {
        std::vector<State>& s;
        ~Pop() { s.pop_back(); }
    } pop{stack_};
    if (obj.has_matrix) transform(matrix_of(obj.matrix));  // a singular matrix puts Cairo's context in an error state; here it is ignored
    switch (obj.type) {
        case SWFR_OBJECT_CONTAINER:
            for (uint32_t i = 0; i < obj.n_children; ++i) draw(obj.children[i], depth + 1);
            break;
        case SWFR_OBJECT_COLOR_TRANSFORM: {
            const auto& slots = store()->cxforms_;
            const auto it = slots.find(obj.id);
            if (it == slots.end()) throw StatusError{SWFR_ERR_NOT_FOUND, "ColorTransformNotFound"};
            stack_.back().lut = compose(stack_.back().lut, it->second);
            for (uint32_t i = 0; i < obj.n_children; ++i) draw(obj.children[i], depth + 1);
            break;
        }
        case SWFR_OBJECT_BLEND_MODE:
            stack_.back().op = blend_operator(obj.id, alpha_modes_);
            for (uint32_t i = 0; i < obj.n_children; ++i) draw(obj.children[i], depth + 1);
            break;
        case SWFR_OBJECT_LAYER:
            draw_layer(obj, depth, obj.id, 255u);
            break;
        case SWFR_OBJECT_FADED_LAYER:
            if (obj.id >= 0x10000u) throw StatusError{SWFR_ERR_INVALID, "FadedLayerId"};
            draw_layer(obj, depth, obj.id & 0xffu, obj.id >> 8);
            break;
        case SWFR_OBJECT_MASKED_LAYER:
            draw_masked_layer(obj, depth);
            break;
        case SWFR_OBJECT_BLURRED_LAYER:
        case SWFR_OBJECT_SHADOWED_LAYER:
        case SWFR_OBJECT_FILTERED_LAYER:
            draw_filtered_layer(obj, depth);
            break;
        case SWFR_OBJECT_SHAPE: {
            const DecodedShape* sh = shape(obj.id, false);
            if (!sh) throw StatusError{SWFR_ERR_NOT_FOUND, "unknown shape id"};
            for (const StyledPath& p : sh->paths) draw_path(p, false, 0.0);
            break;
        }
        case SWFR_OBJECT_MORPH_SHAPE: {
            const DecodedShape* sh = shape(obj.id, true);
            if (!sh) throw StatusError{SWFR_ERR_NOT_FOUND, "unknown morph shape id"};
            for (const StyledPath& p : sh->paths) draw_path(p, true, obj.ratio);
            break;
        }
        default:
            throw StatusError{SWFR_ERR_INVALID, "UnexpectedDisplayObjectType"};
    }
}

// An isolated group ("Isolated layers"): cairo_push_group; the children; cairo_pop_group_to_source; cairo_set_operator;
// cairo_paint.  The children's paths go between a GROUP_BEGIN and a GROUP_END marker whose rectangle is the union of theirs; inside,
// "the surface" is the group's and starts clear -- known here, so a first paint is settled to a SOURCE lerp at once (a group is never
// cut across build pieces: only the single container, colour-transform and blend-mode wrappers around the pieces are).
// With an opacity below 255 (SWFR_OBJECT_FADED_LAYER; DESIGN.md, "Layer opacity") the last call is cairo_paint_with_alpha(opacity / 255.0):
// the END marker carries the fade 255 - opacity in bits 24..31 of its `lerp`.
void FrameBuilder::draw_layer(const swfr_display_object& obj, int depth, uint32_t mode, uint32_t opacity) {
    const uint32_t op = layer_operator(mode, alpha_modes_);
    if (group_depth_ >= SWFR_MAX_LAYER_DEPTH) throw StatusError{SWFR_ERR_CAPACITY, "LayerDepth"};
    const bool parent_clear = surface_clear_;
    const PixelRect parent_drawn = drawn_;
    const size_t begin = paths_.size(), begin_edges = edges_.size(), begin_styles = styles_.size();
    swfr_path m;
    std::memset(&m, 0, sizeof m);
    m.kind = SWFR_PATH_GROUP_BEGIN;
    m.first_edge = uint32_t(edges_.size());
    paths_.push_back(m);
    surface_clear_ = true;
    drawn_ = PixelRect{};
    ++group_depth_;
    for (uint32_t i = 0; i < obj.n_children; ++i) draw(obj.children[i], depth + 1);      // (a throw ends the whole build: nothing to unwind)
    --group_depth_;
    const bool group_clear = surface_clear_;
    drawn_ = parent_drawn;
    // libcairo: painting a still-clear group with OVER or ADD is NOTHING_TO_DO and leaves the parent's "still clear" state alone; under
    // any other operator, and whenever the group was drawn on (even if every pixel of it is zero), the parent counts as drawn
    surface_clear_ = parent_clear && group_clear && (op == SWFR_OP_OVER || op == SWFR_OP_ADD);
    if (opacity == 0u && op != SWFR_OP_ALPHA) {
        // libcairo: cairo_paint_with_alpha(0) returns at once under the nine operators and under ERASE (each is bounded by the mask): no
        // pixel changes and the parent's "still clear" state survives even behind a group that was drawn on.  Nothing is emitted
        surface_clear_ = parent_clear;
        paths_.resize(begin);
        edges_.resize(begin_edges);
        styles_.resize(begin_styles);
        return;
    }
    if (op == SWFR_OP_ALPHA && (opacity == 0u || paths_.size() == begin + 1)) {
        // ALPHA (DEST_IN) is not bounded by its mask or its source: at opacity 0, and with a group no path of which survived, the source
        // is transparent everywhere and the parent surface becomes clear
        paths_.resize(begin);
        edges_.resize(begin_edges);
        styles_.resize(begin_styles);
        emit_clearing_group();
        return;
    }
    if (paths_.size() == begin + 1) {                         // no path survived: a transparent group changes no pixel under these operators
        paths_.pop_back();
        return;
    }
    swfr_path& b = paths_[begin];
    group_rectangle(b, begin, paths_.size(), op);
    m = b;
    m.kind = SWFR_PATH_GROUP_END;
    m.first_edge = uint32_t(edges_.size());
    m.lerp = (op << 8) | ((255u - opacity) << 24);            // (0 < opacity < 255: libcairo's bookkeeping is the plain layer's, above)
    paths_.push_back(m);
}

// The rectangle of a group's markers: the union of the rectangles of paths_[begin + 1 .. end) (the MASK marker among them has none yet:
// all zero, skipped by its kind).  ALPHA ("Erase and alpha modes") takes in everything drawn on the parent surface so far:
// the composite clears the parent wherever the group is transparent, and outside this rectangle the parent is clear already.  The
// parent surface has then been drawn on inside the markers' rectangle, whatever the operator.
void FrameBuilder::group_rectangle(swfr_path& b, size_t begin, size_t end, uint32_t op) {
    PixelRect u;
    for (size_t i = begin + 1; i < end; ++i)
        if (paths_[i].kind != SWFR_PATH_GROUP_MASK) u.add(paths_[i].x_min, paths_[i].y_min, paths_[i].x_max, paths_[i].y_max);
    if (op == SWFR_OP_ALPHA) u.add(drawn_);
    b.x_min = u.x0; b.y_min = u.y0; b.x_max = u.x1; b.y_max = u.y1;
    drawn_.add(u);
}

// An ALPHA layer whose source is transparent everywhere: an empty group over everything drawn on the surface so far, which its END
// clears.  Nothing was drawn: nothing to clear, nothing is emitted (the surface counts as drawn on all the same: the caller)
void FrameBuilder::emit_clearing_group() {
    if (drawn_.empty()) return;
    swfr_path m;
    std::memset(&m, 0, sizeof m);
    m.kind = SWFR_PATH_GROUP_BEGIN;
    m.first_edge = uint32_t(edges_.size());
    m.x_min = drawn_.x0; m.y_min = drawn_.y0; m.x_max = drawn_.x1; m.y_max = drawn_.y1;
    paths_.push_back(m);
    m.kind = SWFR_PATH_GROUP_END;
    m.lerp = uint32_t(SWFR_OP_ALPHA) << 8;
    paths_.push_back(m);
}

// A masked layer ("Masked layers"): cairo_push_group; children[1..]; content = cairo_pop_group; cairo_push_group;
// children[0]; mask = cairo_pop_group; cairo_set_source(content); cairo_set_operator; cairo_mask(mask).  BEGIN; the content's paths;
// MASK; the mask's paths; END(operator), the three markers sharing the union of all member rectangles.  Each half is a group surface of
// its own that starts clear; the pair takes two levels of SWFR_MAX_LAYER_DEPTH from its BEGIN on.
void FrameBuilder::draw_masked_layer(const swfr_display_object& obj, int depth) {
    const uint32_t op = layer_operator(obj.id, alpha_modes_);
    if (obj.n_children == 0) throw StatusError{SWFR_ERR_INVALID, "MaskedLayerWithoutMask"};
    if (group_depth_ + 2 > SWFR_MAX_LAYER_DEPTH) throw StatusError{SWFR_ERR_CAPACITY, "LayerDepth"};
    const bool parent_clear = surface_clear_;
    const PixelRect parent_drawn = drawn_;
    const size_t begin = paths_.size(), begin_edges = edges_.size(), begin_styles = styles_.size();
    swfr_path m;
    std::memset(&m, 0, sizeof m);
    m.kind = SWFR_PATH_GROUP_BEGIN;
    m.first_edge = uint32_t(edges_.size());
    paths_.push_back(m);
    group_depth_ += 2;
    surface_clear_ = true;
    drawn_ = PixelRect{};
    for (uint32_t i = 1; i < obj.n_children; ++i) draw(obj.children[i], depth + 1);
    const bool content_clear = surface_clear_;
    const size_t mask_at = paths_.size();
    m.kind = SWFR_PATH_GROUP_MASK;
    m.first_edge = uint32_t(edges_.size());
    paths_.push_back(m);
    surface_clear_ = true;
    drawn_ = PixelRect{};
    draw(obj.children[0], depth + 1);
    const bool mask_clear = surface_clear_;
    group_depth_ -= 2;
    drawn_ = parent_drawn;
    // libcairo: a still-clear mask is NOTHING_TO_DO under every operator that is bounded by its mask, a still-clear content under OVER
    // and ADD only; the parent's "still clear" state survives exactly then.  Otherwise -- both drawn on, even with every pixel zero --
    // the parent counts as drawn.  ALPHA is not bounded by its mask: never nothing to do
    const bool nothing_to_do = op != SWFR_OP_ALPHA && (mask_clear || (content_clear && (op == SWFR_OP_OVER || op == SWFR_OP_ADD)));
    surface_clear_ = parent_clear && nothing_to_do;
    // a half without a surviving path is transparent: the product mul_un8(C, Ma) is, and changes no pixel under any operator -- but
    // ALPHA, under which the parent surface becomes clear
    if (nothing_to_do || mask_at == begin + 1 || paths_.size() == mask_at + 1) {
        paths_.resize(begin);
        edges_.resize(begin_edges);
        styles_.resize(begin_styles);
        if (op == SWFR_OP_ALPHA) emit_clearing_group();
        return;
    }
    swfr_path& b = paths_[begin];
    group_rectangle(b, begin, paths_.size(), op);
    swfr_path& k = paths_[mask_at];
    k.x_min = b.x_min; k.y_min = b.y_min; k.x_max = b.x_max; k.y_max = b.y_max;
    m = b;
    m.kind = SWFR_PATH_GROUP_END;
    m.first_edge = uint32_t(edges_.size());
    m.lerp = op << 8;
    paths_.push_back(m);
}

// A blurred, shadowed or filtered layer ("Blurred layers", "Shadowed layers", "Filter lists"): cairo_push_group; the children;
// cairo_pop_group; the filters, in order, on the group's surface; cairo_set_source; cairo_set_operator; cairo_paint.  The three types
// differ in where the list comes from: a blurred layer's `id` carries its one blur, a shadowed layer's names a shadow slot, a filtered
// layer's a filter-list slot -- the slots' values at this walk, checked again here.  The children are built -- under the matrix,
// colour-transform chain and blend mode in force -- into a sub-frame of their own: a surface of the frame's size that starts clear,
// with its own layer depth; the list is kept with it for swfr_render.  In the parent the object is one box path over the whole frame
// whose bitmap style names the sub-frame's filtered texture, BLUR_BASE + k: a nearest fetch at 1:1 under full coverage, composited
// with the operator, is the group paint.  The parent surface counts as drawn on behind it (the filtered surface is dirty to Cairo
// whatever it holds).  ALPHA is a group's operator only in the tile pass: the path then sits in a group of its own over the whole
// frame, which the END composites with it.
void FrameBuilder::draw_filtered_layer(const swfr_display_object& obj, int depth) {
    const uint32_t mode = obj.id & 0xffu;
    const uint32_t op = layer_operator(mode, alpha_modes_);      // (a refused mode is reported before a bad filter)
    swfr_filter list[SWFR_MAX_FILTERS];
    swfr_kernel kernels[SWFR_MAX_FILTERS];
    uint32_t n_list = 1;
    std::memset(list, 0, sizeof list);
    std::memset(kernels, 0, sizeof kernels);
    if (obj.type == SWFR_OBJECT_BLURRED_LAYER) {
        list[0].kind = SWFR_FILTER_BLUR;
        list[0].shadow.blur_x = (obj.id >> 8) & 0xffu; list[0].shadow.blur_y = (obj.id >> 16) & 0xffu; list[0].shadow.passes = obj.id >> 24;
        if (!filter_valid(list[0])) throw StatusError{SWFR_ERR_INVALID, "InvalidBlur"};
    } else if (obj.type == SWFR_OBJECT_SHADOWED_LAYER) {
        const uint32_t slot = obj.id >> 8;
        if (slot > 65535u) throw StatusError{SWFR_ERR_INVALID, "InvalidShadow"};
        const auto& slots = store()->shadows_;
        const auto it = slots.find(slot);
        if (it == slots.end()) throw StatusError{SWFR_ERR_NOT_FOUND, "ShadowNotFound"};
        list[0].kind = SWFR_FILTER_SHADOW;
        list[0].shadow = it->second;
        if (!filter_valid(list[0])) throw StatusError{SWFR_ERR_INVALID, "InvalidShadow"};
    } else {
        const uint32_t slot = obj.id >> 8;
        if (slot > 65535u) throw StatusError{SWFR_ERR_INVALID, "InvalidFilter"};
        const auto& slots = store()->filters_;
        const auto it = slots.find(slot);
        if (it == slots.end() || it->second.empty()) throw StatusError{SWFR_ERR_NOT_FOUND, "FiltersNotFound"};
        if (it->second.size() > SWFR_MAX_FILTERS) throw StatusError{SWFR_ERR_CAPACITY, "FilterListLength"};
        n_list = uint32_t(it->second.size());
        for (uint32_t i = 0; i < n_list; ++i) {
            list[i] = it->second[i];
            if (!filter_valid(list[i])) throw StatusError{SWFR_ERR_INVALID, "InvalidFilter"};
            if (list[i].kind != SWFR_FILTER_CONVOLUTION) continue;
            const auto kit = store()->kernels_.find(list[i].shadow.blur_x);      // the kernel is its slot's value at this walk
            if (kit == store()->kernels_.end()) throw StatusError{SWFR_ERR_NOT_FOUND, "KernelNotFound"};
            kernels[i] = kit->second;
            if (!kernel_valid(kernels[i])) throw StatusError{SWFR_ERR_INVALID, "InvalidKernel"};
        }
    }
    if (in_blur_) throw StatusError{SWFR_ERR_NOT_IMPLEMENTED, "NestedBlur"};
    if (parent_) throw StatusError{BLUR_IN_PIECE, "blurred layer in a build piece"};
    if (layers_.size() >= SWFR_MAX_BLUR_LAYERS) throw StatusError{SWFR_ERR_CAPACITY, "BlurLayers"};
    if (op == SWFR_OP_ALPHA && group_depth_ >= SWFR_MAX_LAYER_DEPTH) throw StatusError{SWFR_ERR_CAPACITY, "LayerDepth"};
    // ---- the sub-frame: the walk goes on into fresh arrays
    std::vector<swfr_edge> parent_edges; std::vector<swfr_path> parent_paths; std::vector<swfr_style> parent_styles;
    parent_edges.swap(edges_); parent_paths.swap(paths_); parent_styles.swap(styles_);
    const PixelRect parent_drawn = drawn_;
    const int parent_depth = group_depth_;
    surface_clear_ = true; drawn_ = PixelRect{}; group_depth_ = 0; in_blur_ = true;
    for (uint32_t i = 0; i < obj.n_children; ++i) draw(obj.children[i], depth + 1);      // (a throw ends the whole build: nothing to unwind)
    for (swfr_path& p : paths_) p.lerp = settle_lerp(p.lerp, true);
    layers_.emplace_back();
    BlurLayer& L = layers_.back();
    L.edges.swap(edges_); L.paths.swap(paths_); L.styles.swap(styles_);
    L.type = obj.type; L.n_filters = n_list;
    std::memcpy(L.filters, list, sizeof list);
    std::memcpy(L.kernels, kernels, sizeof kernels);
    edges_.swap(parent_edges); paths_.swap(parent_paths); styles_.swap(parent_styles);
    drawn_ = parent_drawn; group_depth_ = parent_depth; in_blur_ = false;
    // ---- the parent's path
    const int32_t w = int32_t(w_), h = int32_t(h_);
    swfr_path m;
    std::memset(&m, 0, sizeof m);
    m.x_max = w; m.y_max = h;
    if (op == SWFR_OP_ALPHA) {
        m.kind = SWFR_PATH_GROUP_BEGIN;
        m.first_edge = uint32_t(edges_.size());
        paths_.push_back(m);
    }
    swfr_style st;
    std::memset(&st, 0, sizeof st);
    st.kind = SWFR_STYLE_BITMAP;
    st.inv[0] = 1.0; st.inv[3] = 1.0;
    st.bitmap = BLUR_BASE + uint32_t(layers_.size() - 1);
    st.extend = 0; st.filter = 1;
    styles_.push_back(st);
    swfr_path p = m;
    p.kind = SWFR_PATH_BOXES;
    p.first_edge = uint32_t(edges_.size()); p.n_edges = 1;
    p.style = uint32_t(styles_.size() - 1);
    p.lerp = op == SWFR_OP_ALPHA ? 0u : op << 8;
    swfr_edge b;
    std::memset(&b, 0, sizeof b);
    b.x2 = w * 256; b.y2 = h * 256; b.bottom = b.y2; b.dir = 1; b.reserved = int32_t(paths_.size());
    edges_.push_back(b);
    paths_.push_back(p);
    if (op == SWFR_OP_ALPHA) {
        m.kind = SWFR_PATH_GROUP_END;
        m.first_edge = uint32_t(edges_.size());
        m.lerp = op << 8;
        paths_.push_back(m);
    }
    surface_clear_ = false;
    drawn_.add(0, 0, w, h);
}

bool FrameBuilder::transform(const Affine& m) {
    Affine t = m;
    if (!t.invert_cairo()) return false;
    State& st = stack_.back();
    st.ctm = m.then(st.ctm);
    st.inv = st.inv.then(t);
    return true;
}

void FrameBuilder::trace(const StyledPath& p, bool morph, double ratio) {
    const Affine& ctm = stack_.back().ctm;
    auto val = [&](const Coord& c) { return morph ? lerp(c.s, c.e, ratio) : c.s; };
    auto dev = [&](double x, double y) {
        ctm.apply(x, y);
        // 24.8 device coordinates within +-32768 px: beyond that neither Cairo's fixed point nor the kernels' int64 products hold
        if (!(std::fabs(x) <= 32768.0 && std::fabs(y) <= 32768.0)) throw StatusError{SWFR_ERR_INVALID, "geometry outside +-32768 device pixels"};
        return Pt{to_fixed(x), to_fixed(y)};
    };
    path_.clear();
    for (const PathCommand& c : p.commands) {
        switch (c.kind) {
            case PathCommand::MoveTo:
                path_.move_to(dev(val(c.x), val(c.y)));
                break;
            case PathCommand::LineTo:
                path_.line_to(dev(val(c.x), val(c.y)));
                break;
            case PathCommand::CurveTo: {
                // node-canvas quadraticCurveTo: the current point is the quantised device point mapped
                // back to user space; (0,0) stands for "no current point" and selects the control point
                double x = 0, y = 0;
                if (path_.has_current_point()) {
                    Affine inv = ctm;
                    x = from_fixed(path_.current_point().x);
                    y = from_fixed(path_.current_point().y);
                    if (inv.invert()) inv.apply(x, y);
                }
                const double x1 = val(c.cx), y1 = val(c.cy), x2 = val(c.x), y2 = val(c.y);
                if (x == 0 && y == 0) {
                    x = x1;
                    y = y1;
                }
                const double k = 2.0 / 3.0;
                path_.cubic_to(dev(x + k * (x1 - x), y + k * (y1 - y)), dev(x2 + k * (x1 - x2), y2 + k * (y1 - y2)), dev(x2, y2));
                break;
            }
        }
    }
}

void FrameBuilder::draw_path(const StyledPath& p, bool morph, double ratio) {
    if ((!p.has_fill && !p.has_line) || p.commands.empty()) return;
    trace(p, morph, ratio);
    if (p.has_fill) emit_fill(p.fill, morph, ratio);
    if (p.has_line) emit_stroke(p, morph, ratio);
}

bool FrameBuilder::frame_bounds(Pt lo, Pt hi, bool& needs_clip) const {
    if (!(lo.x < hi.x && lo.y < hi.y)) return false;
    int x0 = floor_px(lo.x), y0 = floor_px(lo.y), x1 = ceil_px(hi.x), y1 = ceil_px(hi.y);
    needs_clip = !(x0 >= 0 && y0 >= 0 && x1 <= int(w_) && y1 <= int(h_));
    x0 = std::max(x0, 0);
    y0 = std::max(y0, 0);
    x1 = std::min(x1, int(w_));
    y1 = std::min(y1, int(h_));
    return x0 < x1 && y0 < y1;
}

uint32_t FrameBuilder::push_solid(uint32_t pixel) {
    swfr_style st;
    std::memset(&st, 0, sizeof st);
    st.kind = SWFR_STYLE_SOLID;
    st.pixel = pixel;
    styles_.push_back(st);
    return uint32_t(styles_.size() - 1);
}

void FrameBuilder::emit_polygon(Polygon& poly, bool rectilinear, uint32_t style, bool opaque_solid, int bx0, int by0, int bx1, int by1) {
    const bool lerp_blend = opaque_solid || surface_clear_;
    // Cairo: geometry whose extents miss the operation's rectangle is NOTHING_TO_DO and leaves the surface's "clear" state alone
    // (trim_extents_to_polygon / _to_boxes) -- e.g. a stroke whose approximate extents touch the frame while its outline does
    // not; a rectilinear path that yields no boxes at all counts as drawn (clip_and_composite_boxes)
    if (poly.empty()) {
        if (rectilinear) surface_clear_ = false;
        return;
    }
    swfr_path p;
    std::memset(&p, 0, sizeof p);
    p.first_edge = uint32_t(edges_.size());
    p.fill_rule = even_odd_ ? 1 : 0;
    p.style = style;
    // 2: a lerp only because the surface is still clear (settled by build()).  A blended path is never a lerp -- an opaque colour under
    // MULTIPLY is not "opaque" for any shortcut -- except that Cairo turns ADD on a still-clear surface into SOURCE, as it does OVER
    // (inside a layer the surface is the group's, whose state this walk knows: settled here)
    const uint32_t op = stack_.back().op;
    const uint32_t first = group_depth_ ? 1u : 2u;
    if (op == SWFR_OP_OVER) p.lerp = opaque_solid ? 1 : (surface_clear_ ? first : 0);
    else if (op == SWFR_OP_ADD) p.lerp = surface_clear_ ? (group_depth_ ? 1u : ((op << 8) | 2u)) : (op << 8);
    else p.lerp = op << 8;
    (void)lerp_blend;
    // converter rectangle: the polygon's extents inside the operation's bounded rectangle (the frame for fills)
    p.x_min = std::max(floor_px(poly.ext_min().x), std::max(bx0, 0));
    p.y_min = std::max(floor_px(poly.ext_min().y), std::max(by0, 0));
    p.x_max = std::min(ceil_px(poly.ext_max().x), std::min(bx1, int(w_)));
    p.y_max = std::min(ceil_px(poly.ext_max().y), std::min(by1, int(h_)));
    if (p.x_min >= p.x_max || p.y_min >= p.y_max) return;
    surface_clear_ = false;
    if (rectilinear) {
        p.kind = SWFR_PATH_BOXES;
        rectilinear_to_boxes(poly, even_odd_, edges_);
        // the box stroker's polygon is not clipped (see emit_stroke): a box may reach far past the frame, even past +-2^23 in 24.8
        // (a path point near +-32768 px plus the half line width).  Only the converter rectangle is painted (Cairo's compositor clips
        // the boxes to it), so the boxes are clamped to it and those that miss it are dropped.  Aliased: every box is rounded to whole
        // pixels first (a path whose boxes all round away has drawn, like one without boxes: the surface is no longer clear)
        const fixed_t cx0 = fixed_t(p.x_min) * 256, cy0 = fixed_t(p.y_min) * 256, cx1 = fixed_t(p.x_max) * 256, cy1 = fixed_t(p.y_max) * 256;
        size_t out = p.first_edge;
        for (size_t k = p.first_edge; k < edges_.size(); ++k) {
            swfr_edge b = edges_[k];
            if (aliased_) round_box_to_pixels(b);
            b.x1 = std::max(b.x1, cx0); b.x2 = std::min(b.x2, cx1);
            b.y1 = std::max(b.y1, cy0); b.y2 = std::min(b.y2, cy1);
            if (b.x1 >= b.x2 || b.y1 >= b.y2) continue;
            b.top = b.y1; b.bottom = b.y2;
            edges_[out++] = b;
        }
        edges_.resize(out);
    } else {
        p.kind = SWFR_PATH_TOR;
        edges_.insert(edges_.end(), poly.edges().begin(), poly.edges().end());
    }
    p.n_edges = uint32_t(edges_.size()) - p.first_edge;
    if (p.n_edges) {
        for (uint32_t k = p.first_edge; k < p.first_edge + p.n_edges; ++k) edges_[k].reserved = int32_t(paths_.size());   // owning path: the device bins by it
        paths_.push_back(p);
        drawn_.add(p.x_min, p.y_min, p.x_max, p.y_max);
    } else edges_.resize(p.first_edge);
}

void FrameBuilder::emit_fill(const OwnedFill& f, bool morph, double ratio) {
    const swfr_fill_style& s = f.style;
    uint32_t style_index = 0;
    bool opaque_solid = false;
    // context.save(); <source>; fill(); context.restore()  (canvas-renderer.ts:292-336)
    if (s.type == SWFR_FILL_SOLID) {
        const uint32_t px = premultiplied_pixel(morph_color(cx(s.color), cx(s.morph_color), morph, ratio));
        if ((px >> 24) == 0 && clear_source_is_noop()) return;  // Cairo: OVER (and ADD) with a clear source is a no-op
        opaque_solid = (px >> 24) == 0xff;
        style_index = push_solid(px);
    } else if (s.type == SWFR_FILL_BITMAP) {
        auto it = store()->bitmaps_.find(s.bitmap_id);
        if (it == store()->bitmaps_.end()) throw StatusError{SWFR_ERR_NOT_FOUND, "BitmapNotFound: " + std::to_string(s.bitmap_id)};
        swfr_style st;
        std::memset(&st, 0, sizeof st);
        st.kind = SWFR_STYLE_BITMAP;
        // context.save(); transform(fill.matrix): the pattern matrix is the inverse CTM at fill() time
        Affine fm = matrix_of(s.matrix);
        if (!fm.invert_cairo()) return;
        const Affine inv = stack_.back().inv.then(fm);
        const double m[6] = {inv.xx, inv.yx, inv.xy, inv.yy, inv.x0, inv.y0};
        std::memcpy(st.inv, m, sizeof m);
        const int32_t lut = stack_.back().lut;
        if (lut >= 0 && it->second.captured) throw StatusError{SWFR_ERR_NOT_IMPLEMENTED, "NotImplementedCapturedBitmapTransform"};
        st.bitmap = lut < 0 ? s.bitmap_id : VARIANT_BASE + variant_of(s.bitmap_id, lut);
        st.extend = s.pad ? 2 : s.repeating ? 1 : 0;               // (pad and repeating together are refused when the shape is registered)
        st.filter = s.filter;                                      // 0 CAIRO_FILTER_GOOD, 1 CAIRO_FILTER_NEAREST (above 1: refused with the shape)
        styles_.push_back(st);
        style_index = uint32_t(styles_.size() - 1);
    } else {
        // Radial == focal with focalPoint 0 (decode-swf-shape.ts:127-133); createRadialGradient(
        // f*16384, 0, 0, 0, 0, 16384) under fill.matrix (canvas-renderer.ts:320-331).  Linear gradients
        // throw NotImplementedFillStyle in the reference (:332-333); here they are the documented
        // extension createLinearGradient(-16384, 0, 16384, 0).
        if (f.stops.size() > SWFR_MAX_STOPS) throw StatusError{SWFR_ERR_CAPACITY, "too many gradient stops"};
        swfr_style st;
        std::memset(&st, 0, sizeof st);
        Affine fm = matrix_of(s.matrix);
        if (!fm.invert_cairo()) return;
        const Affine inv = stack_.back().inv.then(fm);
        const double m[6] = {inv.xx, inv.yx, inv.xy, inv.yy, inv.x0, inv.y0};
        std::memcpy(st.inv, m, sizeof m);
        const double R = 16384.0;
        // cairo_pattern_set_extend of the SWF spread (0 pad, 1 reflect, 2 repeat) -- beyond the reference, which never reads the
        // field.  A linear gradient is the float64 extension: next to a repeat seam a +-1 LSB model can land a whole colour away,
        // so a spread one is refused
        st.extend = s.spread == 1 ? 2u : s.spread == 2 ? 1u : 0u;
        // (SWFR_FLAG_LINEAR_PIXMAN: pixman's own evaluation, SWFR_STYLE_LINEAR_PIXMAN, which has every spread)
        if (s.type == SWFR_FILL_LINEAR_GRADIENT && st.extend && !linear_pixman_) throw StatusError{SWFR_ERR_NOT_IMPLEMENTED, "NotImplementedGradientSpread"};
        if (s.type == SWFR_FILL_LINEAR_GRADIENT) {
            st.kind = linear_pixman_ ? SWFR_STYLE_LINEAR_PIXMAN : SWFR_STYLE_LINEAR;
            st.c0x = -R; st.c1x = R;
        } else {
            st.kind = SWFR_STYLE_RADIAL;
            const double focal = s.type == SWFR_FILL_FOCAL_GRADIENT ? s.focal_point / 256.0 : 0.0;
            st.c0x = lerp(0, R, focal);
            st.r0 = 0; st.r1 = R;
        }
        // stops sorted by offset, stable (cairo_pattern_add_color_stop keeps them ordered)
        std::vector<swfr_color_stop> stops = f.stops;
        for (swfr_color_stop& c : stops) { c.color = cx(c.color); c.morph_color = cx(c.morph_color); }
        std::stable_sort(stops.begin(), stops.end(), [](const swfr_color_stop& a, const swfr_color_stop& b) { return a.ratio < b.ratio; });
        st.n_stops = uint32_t(stops.size());
        for (size_t i = 0; i < stops.size(); ++i) {
            const Css c = css_color(stops[i].color.r / 255.0, stops[i].color.g / 255.0, stops[i].color.b / 255.0, stops[i].color.a / 255.0);
            st.stop_offset[i] = float(stops[i].ratio / 255.0);
            st.stop_rgba[i][0] = float(c.r / 255.0);
            st.stop_rgba[i][1] = float(c.g / 255.0);
            st.stop_rgba[i][2] = float(c.b / 255.0);
            st.stop_rgba[i][3] = float(c.a / 255.0);
        }
        // a gradient whose stops are all transparent is a clear source (_cairo_pattern_is_clear -> _gradient_is_clear): OVER with
        // it is a no-op that leaves the surface's "clear" state alone, like the transparent solid above
        if (clear_source_is_noop() && std::all_of(stops.begin(), stops.end(), [](const swfr_color_stop& c) { return c.color.a == 0; })) return;
        styles_.push_back(st);
        style_index = uint32_t(styles_.size() - 1);
    }
    if (path_.empty_extents()) return;
    // the operation's bounded rectangle: path extents rounded out (the mask), inside the frame, inside the source's extents
    const Pt plo = path_.box_min(), phi = path_.box_max();
    if (!(plo.x < phi.x && plo.y < phi.y)) return;  // nothing to do: surface stays clear
    int x0 = floor_px(plo.x), y0 = floor_px(plo.y), x1 = ceil_px(phi.x), y1 = ceil_px(phi.y);
    const int mask_w = x1 - x0, mask_h = y1 - y0;
    x0 = std::max(x0, 0);
    y0 = std::max(y0, 0);
    x1 = std::min(x1, int(w_));
    y1 = std::min(y1, int(h_));
    if (s.type == SWFR_FILL_BITMAP && !s.repeating && !s.pad) {
        // OVER is bounded by its source (_cairo_pattern_get_extents of an EXTEND_NONE surface pattern; a repeating or padded one is
        // unbounded): the bitmap's rectangle in
        // device space; an axis the filter magnifies is padded by half a source pixel and rounded to the nearest pixel edge,
        // the others are rounded out.  CAIRO_FILTER_NEAREST pads by 0.004 source pixels ("this avoids rounding errors") and rounds
        // to the nearest pixel edge on both axes, whatever the scale
        const swfr_style& st = styles_[style_index];
        Affine pm;
        pm.xx = st.inv[0]; pm.yx = st.inv[1]; pm.xy = st.inv[2]; pm.yy = st.inv[3]; pm.x0 = st.inv[4]; pm.y0 = st.inv[5];
        const BitmapInfo& bi = store()->bitmaps_.find(s.bitmap_id)->second;
        double sx0 = 0, sy0 = 0, sx1 = bi.width, sy1 = bi.height;
        bool round_x = false, round_y = false;
        if (st.filter == 1) {
            sx0 -= 0.004; sx1 += 0.004; sy0 -= 0.004; sy1 += 0.004;
            round_x = round_y = true;
        } else {
            if (std::hypot(pm.xx, pm.yx) < 1.0) { sx0 -= 0.5; sx1 += 0.5; round_x = true; }
            if (std::hypot(pm.xy, pm.yy) < 1.0) { sy0 -= 0.5; sy1 += 0.5; round_y = true; }
        }
        Affine im = pm;
        if (im.invert_cairo()) {
            double bx0 = 0, by0 = 0, bx1 = 0, by1 = 0;
            for (int k = 0; k < 4; ++k) {
                double x = (k & 1) ? sx1 : sx0, y = (k & 2) ? sy1 : sy0;
                im.apply(x, y);
                if (!k || x < bx0) bx0 = x;
                if (!k || x > bx1) bx1 = x;
                if (!k || y < by0) by0 = y;
                if (!k || y > by1) by1 = y;
            }
            if (!round_x) { bx0 -= 0.5; bx1 += 0.5; }
            if (!round_y) { by0 -= 0.5; by1 += 0.5; }
            bx0 = std::floor(bx0 + 0.5); by0 = std::floor(by0 + 0.5); bx1 = std::floor(bx1 + 0.5); by1 = std::floor(by1 + 0.5);
            if (x0 < bx0) x0 = int(bx0);
            if (y0 < by0) y0 = int(by0);
            if (x1 > bx1) x1 = int(bx1);
            if (y1 > by1) y1 = int(by1);
        }
    }
    if (x0 >= x1 || y0 >= y1) return;                   // nothing to do: surface stays clear
    const bool needs_clip = mask_w > x1 - x0 || mask_h > y1 - y0;
    Polygon& poly = poly_;                            // (reused: its edge vector keeps its capacity from shape to shape)
    const Pt lo{fixed_t(x0) * 256, fixed_t(y0) * 256}, hi{fixed_t(x1) * 256, fixed_t(y1) * 256};  // the limits are the bounded rectangle
    poly.reset(needs_clip, lo, hi);
    if (needs_clip) fill_to_polygon_clipped(path_, poly, lo, hi); else fill_to_polygon(path_, poly);
    emit_polygon(poly, path_.fill_is_rectilinear(), style_index, opaque_solid, x0, y0, x1, y1);
}

void FrameBuilder::emit_stroke(const StyledPath& p, bool morph, double ratio) {
    if (p.fill.style.type != SWFR_FILL_SOLID) throw StatusError{SWFR_ERR_NOT_IMPLEMENTED, "NotImplementedLineStyle"};
    State& st = stack_.back();
    const double width = morph ? lerp(p.width, p.morph_width, ratio) : double(p.width);
    if (width > 0) st.line_width = width;  // node-canvas ignores non-positive widths
    const uint32_t px = premultiplied_pixel(morph_color(cx(p.fill.style.color), cx(p.fill.style.morph_color), morph, ratio));
    if (morph) st.cap = st.join = 1;  // lineCap = lineJoin = "round" (canvas-renderer.ts:263-264)
    if ((px >> 24) == 0 && clear_source_is_noop()) return;
    if (path_.empty_extents()) return;
    // _cairo_compositor_stroke: a pen that degenerates to one vertex (line width <= tolerance/2 = 0.05 device pixels under the CTM)
    // paints nothing, whatever the stroker; the surface stays untouched
    if (stroke_pen_vertices(st.line_width, st.ctm) <= 1) return;
    // approximate stroke extents: path box grown by the style's maximum distance from the path
    double expansion = 0.5;
    if (st.cap == 2) expansion = M_SQRT1_2;
    if (st.join == 0 && !path_.stroke_is_rectilinear() && expansion < M_SQRT2 * 10.0) expansion = M_SQRT2 * 10.0;
    expansion *= st.line_width;
    const Affine& c = st.ctm;
    const double eps = 1.0 / 256.0, det = c.det();
    const bool unity = std::fabs(det * det - 1.0) < eps &&
                       ((std::fabs(c.xy) < eps && std::fabs(c.yx) < eps) || (std::fabs(c.xx) < eps && std::fabs(c.yy) < eps));
    const double gx = unity ? expansion : expansion * std::hypot(c.xx, c.xy);
    const double gy = unity ? expansion : expansion * std::hypot(c.yy, c.yx);
    Pt lo = path_.box_min(), hi = path_.box_max();
    lo.x -= to_fixed(gx); lo.y -= to_fixed(gy);
    hi.x += to_fixed(gx); hi.y += to_fixed(gy);
    bool needs_clip = false;
    if (!frame_bounds(lo, hi, needs_clip)) return;
    // the operation is bounded by these extents (rounded out, inside the frame): what the stroker produces beyond them is not painted
    const int bx0 = std::max(floor_px(lo.x), 0), by0 = std::max(floor_px(lo.y), 0);
    const int bx1 = std::min(ceil_px(hi.x), int(w_)), by1 = std::min(ceil_px(hi.y), int(h_));
    const Pt frame_lo{0, 0}, frame_hi{fixed_t(w_) * 256, fixed_t(h_) * 256};
    StrokeParams sp;
    sp.line_width = st.line_width;
    sp.cap = st.cap;
    sp.join = st.join;
    const bool opaque = (px >> 24) == 0xff;
    // strokes are filled non-zero regardless of the configured fill rule
    const bool saved = even_odd_;
    even_odd_ = false;
    Polygon& poly = poly_;
    bool done = false;
    if (path_.stroke_is_rectilinear()) {
        // Cairo's box stroker when it accepts the style: the union of one box per segment, painted like a rectilinear fill.  Its
        // boxes are NOT clipped against the frame first: a stroke whose boxes all lie outside is then "boxes that miss the operation's
        // rectangle" (nothing drawn, the surface keeps its clear state) and not "no boxes at all" (which counts as drawn) -- found by
        // the soak (mixed 7100/2196: the next translucent fill is then still composited with the SOURCE rule).  emit_polygon decides
        // on these unclipped boxes, then clamps them to the frame
        poly.reset(false, frame_lo, frame_hi);
        if (stroke_rectilinear_to_boxes(path_, sp, st.ctm, poly)) {
            emit_polygon(poly, true, push_solid(px), opaque, bx0, by0, bx1, by1);
            done = true;
        }
    }
    if (!done) {
        poly.reset(needs_clip, frame_lo, frame_hi);
        if (needs_clip) {
            sp.has_bounds = true;
            sp.bounds_lo = Pt{frame_lo.x - to_fixed(gx), frame_lo.y - to_fixed(gy)};
            sp.bounds_hi = Pt{frame_hi.x + to_fixed(gx), frame_hi.y + to_fixed(gy)};
        }
        if (!stroke_to_polygon(path_, sp, st.ctm, poly)) {
            even_odd_ = saved;
            return;                                            // singular CTM: nothing can be stroked
        }
        emit_polygon(poly, false, push_solid(px), opaque, bx0, by0, bx1, by1);
    }
    even_odd_ = saved;
}

}  // namespace swfr
