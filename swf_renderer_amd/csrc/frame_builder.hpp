// frame_builder.hpp -- host scene walk: Stage -> painter-ordered edge list + path/style tables.
//
// Mirrors CanvasRenderer (ts/src/lib/renderers/canvas-renderer.ts:61-350): reset CTM, clear,
// scale(1/20), matrix stack over containers/shapes/morph shapes, per path beginPath + commands +
// fill() / stroke().  Instead of calling a Canvas it emits what the GPU scan converter consumes.
#pragma once

#include <condition_variable>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/swfr.h"
#include "geometry.hpp"
#include "shape_decoder.hpp"

namespace swfr {

struct BitmapInfo {
    uint32_t width = 0, height = 0;
    bool captured = false;                           // made on the device (swfr_capture_bitmap, swfr_blur_bitmap): no straight texels to transform
};

// The sub-frame of a blurred layer (SWFR_OBJECT_BLURRED_LAYER), a shadowed one (SWFR_OBJECT_SHADOWED_LAYER) or a filtered one
// (SWFR_OBJECT_FILTERED_LAYER): what its children build as a frame of their own, and its filter list.  The parent frame samples the
// rendered, filtered sub-frame as texture BLUR_BASE + k, k the layer's index in FrameBuilder::layers().
struct BlurLayer {
    std::vector<swfr_edge> edges;
    std::vector<swfr_path> paths;
    std::vector<swfr_style> styles;
    // the ordered filters, as the walk read them: a blurred layer's one blur entry made of its `id`, a shadowed layer's one shadow
    // entry (its slot's value), a filtered layer's slot's list
    uint32_t type = 0;                                // the display-object type the layer came from
    uint32_t n_filters = 0;                           // 1..SWFR_MAX_FILTERS
    swfr_filter filters[SWFR_MAX_FILTERS]{};
    swfr_kernel kernels[SWFR_MAX_FILTERS]{};          // entry i's kernel as the walk read it from its slot, where entry i is a convolution
};
constexpr uint32_t BLUR_BASE = SWFR_BLUR_BASE;

struct StatusError {
    int code;
    std::string message;
};

// A chain of colour transforms as four 256-entry tables, channel-major (r, g, b, a): the value a straight channel c takes is lut[ch][c].
struct ColorLut {
    uint8_t t[4][256];
};
// A bitmap fill under a non-identity chain: the frame's bitmap style then names texture VARIANT_BASE + k of the frame's variants().
struct TextureVariant {
    uint32_t bitmap;
    ColorLut lut;
};
constexpr uint32_t VARIANT_BASE = 65536;         // (registered bitmap ids are below it)

// A union of pixel rectangles; empty until the first is added
struct PixelRect {
    int32_t x0 = INT32_MAX, y0 = INT32_MAX, x1 = INT32_MIN, y1 = INT32_MIN;
    bool empty() const { return x0 >= x1 || y0 >= y1; }
    void add(int32_t ax0, int32_t ay0, int32_t ax1, int32_t ay1) {
        if (ax0 >= ax1 || ay0 >= ay1) return;                  // (an empty rectangle holds no pixel)
        x0 = ax0 < x0 ? ax0 : x0; y0 = ay0 < y0 ? ay0 : y0; x1 = ax1 > x1 ? ax1 : x1; y1 = ay1 > y1 ? ay1 : y1;
    }
    void add(const PixelRect& r) { add(r.x0, r.y0, r.x1, r.y1); }
};

// swfr_set_color_transform's check: eight values in the int16 range
bool color_transform_valid(const swfr_color_transform& ct);
// swfr_set_shadow's and swfr_shadow_bitmap's check (swfr.h, swfr_shadow: the ranges, known flags, not both)
bool shadow_valid(const swfr_shadow& s);
// the premultiplied ARGB pixel of cairo_set_source_rgba(r / 255, g / 255, b / 255, a / 255), from the bytes directly
uint32_t shadow_color_pixel(const swfr_rgba8& c);
// swfr_set_filters' check of one entry (swfr.h, swfr_filter): a known kind; a blur entry's box and passes in range and its other fields
// zero; a shadow entry as shadow_valid has it; a convolution entry's slot (shadow.blur_x) below 65536 and its other fields zero
bool filter_valid(const swfr_filter& f);
// swfr_set_kernel's and swfr_convolve_bitmap's check (swfr.h, swfr_kernel): both dimensions 1..SWFR_MAX_KERNEL_DIM, sum |tap| <= 8 388 607
bool kernel_valid(const swfr_kernel& k);

// Frames with many top-level display objects are built by several threads: the children are cut into contiguous ranges, every range
// is walked by a worker builder of its own (same code, its own output arrays), and the pieces are joined in painter's order.  The one
// thing a display object's output depends on besides itself -- whether the surface is still clear, which turns the first translucent
// paint into a SOURCE-rule lerp -- is marked in the paths (`lerp` = 2) and settled when the pieces are joined.
class FrameBuilder {
public:
    FrameBuilder(uint32_t width, uint32_t height, bool even_odd, bool aliased = false, bool linear_pixman = false, bool alpha_modes = false);   // aliased: SWFR_FLAG_ANTIALIAS_NONE
    ~FrameBuilder();
    FrameBuilder(const FrameBuilder&) = delete;
    FrameBuilder& operator=(const FrameBuilder&) = delete;
    void set_threads(int n) { threads_ = n; }          // 0 / 1: single thread; default: SWFR_BUILD_THREADS or min(8, cores)

    uint32_t add_shape(DecodedShape s) { shapes_.push_back(std::move(s)); return uint32_t(shapes_.size() - 1); }
    uint32_t add_morph_shape(DecodedShape s) { morphs_.push_back(std::move(s)); return uint32_t(morphs_.size() - 1); }
    void add_bitmap(uint32_t id, BitmapInfo info) { bitmaps_[id] = info; }
    void set_color_transform(uint32_t slot, const swfr_color_transform* ct) { if (ct) cxforms_[slot] = *ct; else cxforms_.erase(slot); }
    void set_shadow(uint32_t slot, const swfr_shadow* sh) { if (sh) shadows_[slot] = *sh; else shadows_.erase(slot); }
    void set_filters(uint32_t slot, const swfr_filter* f, uint32_t count) { if (f && count) filters_[slot].assign(f, f + count); else filters_.erase(slot); }
    void set_kernel(uint32_t slot, const swfr_kernel* k) { if (k) kernels_[slot] = *k; else kernels_.erase(slot); }
    const DecodedShape* shape(uint32_t id, bool morph) const;

    // Throws StatusError.  Results stay valid until the next build().
    void build(const swfr_stage& stage);
    const std::vector<swfr_edge>& edges() const { return edges_; }
    const std::vector<swfr_path>& paths() const { return paths_; }
    const std::vector<swfr_style>& styles() const { return styles_; }
    const std::vector<TextureVariant>& variants() const { return variants_; }   // textures VARIANT_BASE + k of the bitmap styles, first-use order
    const std::vector<BlurLayer>& layers() const { return layers_; }            // the sub-frames of the frame's blurred layers, in painter's order
    void set_bitmap_captured(uint32_t id) { const auto it = bitmaps_.find(id); if (it != bitmaps_.end()) it->second.captured = true; }

private:
    struct State {
        Affine ctm;
        Affine inv;               // Cairo keeps the inverse beside the CTM and updates it factor by factor (_cairo_gstate_transform)
        double line_width = 1.0;  // node-canvas creates its context with line width 1
        int cap = 0, join = 0;
        int32_t lut = -1;         // colour-transform chain: index into luts_, -1 identity
        uint32_t op = 0;          // blend mode of the innermost SWFR_OBJECT_BLEND_MODE wrapper as a path operator (SWFR_OP_*), 0: OVER
    };
    void draw(const swfr_display_object& obj, int depth);
    void draw_layer(const swfr_display_object& obj, int depth, uint32_t mode, uint32_t opacity);
    void draw_masked_layer(const swfr_display_object& obj, int depth);
    void draw_filtered_layer(const swfr_display_object& obj, int depth);
    void group_rectangle(swfr_path& b, size_t begin, size_t end, uint32_t op);   // the markers' rectangle of the group paths_[begin .. end)
    void emit_clearing_group();                                // an ALPHA layer with a transparent source: the surface drawn so far becomes clear
    void draw_path(const StyledPath& p, bool morph, double ratio);
    void trace(const StyledPath& p, bool morph, double ratio);
    void emit_fill(const OwnedFill& f, bool morph, double ratio);
    void emit_stroke(const StyledPath& p, bool morph, double ratio);
    void emit_polygon(Polygon& poly, bool rectilinear, uint32_t style, bool opaque_solid, int bx0 = 0, int by0 = 0, int bx1 = INT32_MAX, int by1 = INT32_MAX);
    uint32_t push_solid(uint32_t pixel);
    // Cairo drops a drawing operation with a clear source only under OVER and ADD; under the other operators it changes no pixel
    // either but is an operation like any other: the surface no longer counts as clear behind it
    bool clear_source_is_noop() const { return stack_.back().op == SWFR_OP_OVER || stack_.back().op == SWFR_OP_ADD; }
    swfr_rgba8 cx(const swfr_rgba8& c) const;                  // the current chain applied to a straight colour
    int32_t compose(int32_t outer, const swfr_color_transform& inner);   // chain `outer` after `inner`: an index into luts_ (-1: identity)
    uint32_t variant_of(uint32_t bitmap, int32_t lut);         // this builder's texture index of (bitmap, chain)
    bool frame_bounds(Pt lo, Pt hi, bool& needs_clip) const;
    bool transform(const Affine& m);  // context.transform(m); false: singular
    static Affine matrix_of(const swfr_matrix& m);

    // ---- multi-threaded build
    struct Pool;                                         // the worker threads (created on first use)
    // worker: kids [lo, hi), inside the single wrappers `wraps` (outermost first), into this builder's arrays
    void build_range(const std::vector<const swfr_display_object*>& wraps, const swfr_display_object* kids, uint32_t lo, uint32_t hi);
    void copy_piece(FrameBuilder& dst, size_t edge_off, size_t path_off, size_t style_off, bool clear_at_start, const std::vector<uint32_t>& variant_map) const;
    const FrameBuilder* store() const { return parent_ ? parent_ : this; }  // where shapes and bitmaps are registered
    const FrameBuilder* parent_ = nullptr;
    std::unique_ptr<Pool> pool_;
    int threads_ = -1;
    bool failed_ = false;
    StatusError failure_{0, ""};

    uint32_t w_, h_;
    bool even_odd_;
    bool aliased_;
    bool linear_pixman_;     // SWFR_FLAG_LINEAR_PIXMAN: linear gradient fills become SWFR_STYLE_LINEAR_PIXMAN styles
    std::vector<DecodedShape> shapes_, morphs_;
    std::map<uint32_t, BitmapInfo> bitmaps_;
    std::vector<State> stack_;
    DevicePath path_;
    Polygon poly_;
    bool alpha_modes_;       // SWFR_FLAG_ALPHA_MODES: the blend modes erase and alpha are accepted (SWFR_OP_ERASE, SWFR_OP_ALPHA)
    PixelRect drawn_;        // of the surface being drawn on: the union of the rectangles of the paths and group markers emitted onto it
    bool surface_clear_ = true;   // of the surface being drawn on: the frame's, or inside a SWFR_OBJECT_LAYER the innermost group's
    int group_depth_ = 0;         // open layers (at most SWFR_MAX_LAYER_DEPTH)
    std::vector<swfr_edge> edges_;
    std::vector<swfr_path> paths_;
    std::vector<swfr_style> styles_;
    std::vector<BlurLayer> layers_;   // blurred layers met so far (at most SWFR_MAX_BLUR_LAYERS); always built by one walk (build)
    bool in_blur_ = false;            // the walk is inside a blurred layer: edges_, paths_ and styles_ are the sub-frame's
    // colour transforms: the slots (set on the handle's builder), the chains of this walk (deduplicated by content) and the
    // textures its bitmap styles ask for (deduplicated by (bitmap, chain))
    std::map<uint32_t, swfr_color_transform> cxforms_;
    std::map<uint32_t, swfr_shadow> shadows_;   // the shadow slots (set on the handle's builder)
    std::map<uint32_t, std::vector<swfr_filter>> filters_;   // the filter-list slots, likewise
    std::map<uint32_t, swfr_kernel> kernels_;   // the convolution-kernel slots, likewise
    std::vector<ColorLut> luts_;
    std::map<std::string, int32_t> lut_index_;                 // table bytes -> index into luts_
    std::map<std::pair<int32_t, std::string>, int32_t> compose_memo_;   // (outer chain, inner transform bytes) -> chain
    std::map<std::pair<uint32_t, int32_t>, uint32_t> variant_index_;
    std::vector<TextureVariant> variants_;
};

}  // namespace swfr
