/*
 * swfr.h -- C-ABI of libswfr.so, the MI355X-native SWF vector rasterizer.
 *
 * This is the drop-in boundary for the reference's render(Stage) -> RGBA path.  The reference
 * (open-flash/swf-renderer) has no FFI for a rasterizer; its seam is the trait/interface layer,
 * and each entry point below names the reference interface it replaces:
 *
 *   swfr_create / swfr_destroy      HeadlessGfxRenderer::new(&instance, w, h)   rs/src/headless_renderer.rs:60-64
 *                                   new NodeCanvasRenderer(width, height)       ts/src/lib/renderers/node-canvas-renderer.ts:11-15
 *                                   createRenderer / destroyRenderer (handles)  rs/src/wasm.rs:60-76
 *   swfr_register_shape             ClientAssetStore::register_shape            rs/src/asset.rs:9-12
 *                                   (decode: ts/src/lib/shape/decode-swf-shape.ts:22-39)
 *   swfr_register_morph_shape       ClientAssetStore::register_morph_shape      rs/src/asset.rs:9-12
 *                                   (decode: ts/src/lib/shape/decode-swf-morph-shape.ts:21-41)
 *   swfr_register_bitmap(_tag)      Renderer.addBitmap(tag)                     ts/src/lib/renderer.ts:4-8,
 *                                   ts/src/lib/renderers/node-canvas-bitmap-service.ts:14-37
 *   swfr_render                     SwfRenderer::render(&mut self, Stage)       rs/src/swf_renderer.rs:3-5
 *                                   Renderer.render(stage)                      ts/src/lib/renderer.ts:4-8
 *                                   (scene walk: ts/src/lib/renderers/canvas-renderer.ts:69-350)
 *   swfr_read_image                 HeadlessGfxRenderer::get_image() -> Image   rs/src/headless_renderer.rs:233-244,
 *                                   Image{meta{width,height,stride},data}       rs/src/renderer.rs:88-103
 *   swfr_last_error                 Result<_, &'static str> / thrown Error      rs/src/headless_renderer.rs:64,233
 *
 * Conventions mirrored from the reference: definitions are borrowed for the call and copied
 * (rs/src/renderer.rs:24-64); render is synchronous and returns after the GPU is idle
 * (rs/src/headless_renderer.rs:703-712); one handle = one thread at a time; errors are an int
 * status plus a per-handle message, nothing is thrown across the boundary.
 *
 * Types mirror swf-tree 0.8 as evidenced by the reference fixtures (tests/<set>/<name>/ast.json).
 * Plain C: pointers + sizes only, no C++ or torch types.
 */
#ifndef SWFR_H
#define SWFR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SWFR_ABI_VERSION 1

typedef struct swfr_renderer swfr_renderer;               /* opaque handle */

enum {
    SWFR_OK = 0,
    SWFR_ERR_INVALID = 1,          /* bad argument / malformed definition (reference: "Invalid fill ID" etc.) */
    SWFR_ERR_NOT_IMPLEMENTED = 2,  /* reference throws NotImplementedFillStyle / NotImplementedLineStyle */
    SWFR_ERR_NOT_FOUND = 3,        /* unknown shape / bitmap id (reference: BitmapNotFound) */
    SWFR_ERR_NO_DEVICE = 4,        /* no HIP device, or a host-only handle was asked to rasterize */
    SWFR_ERR_DEVICE = 5,           /* HIP runtime error */
    SWFR_ERR_CAPACITY = 6          /* a capacity limit of the scan converter: more than 8192 active edges of one path in a pixel row (or
                                      starting at one sample row), or a limit of the replay of Cairo's
                                      edge-list order for coincident edges (swfr_get_stats) -- the frame is refused, never approximated */
};

/* ---- swf-tree value types ---------------------------------------------------------------- */
typedef struct { uint8_t r, g, b, a; } swfr_rgba8;                          /* StraightSRgba8 */
typedef struct { int32_t x_min, x_max, y_min, y_max; } swfr_rect;           /* twips */
typedef struct {                                                            /* swf_tree::Matrix */
    int32_t scale_x, scale_y, rotate_skew0, rotate_skew1;                   /* Sfixed16P16 epsilons */
    int32_t translate_x, translate_y;                                       /* twips */
} swfr_matrix;

enum { SWFR_FILL_SOLID = 0, SWFR_FILL_LINEAR_GRADIENT = 1, SWFR_FILL_RADIAL_GRADIENT = 2,
       SWFR_FILL_FOCAL_GRADIENT = 3, SWFR_FILL_BITMAP = 4 };

typedef struct { uint8_t ratio; swfr_rgba8 color; swfr_rgba8 morph_color; } swfr_color_stop;

typedef struct {
    uint32_t type;                       /* SWFR_FILL_* */
    swfr_rgba8 color, morph_color;       /* solid (morph_color: DefineMorphShape only) */
    swfr_matrix matrix;                  /* gradients, bitmap */
    uint32_t n_stops;                    /* gradients */
    const swfr_color_stop *stops;
    int32_t focal_point;                 /* focal gradient, Sfixed8P8 epsilons */
    uint32_t bitmap_id;                  /* bitmap */
    uint8_t repeating, smoothed;
    uint8_t spread;                      /* gradients: the SWF GradientSpread number -- 0 pad, 1 reflect, 2 repeat: the gradient's Cairo pattern
                                            with cairo_pattern_set_extend(PAD | REFLECT | REPEAT).  Anything else: SWFR_ERR_INVALID,
                                            "UnknownGradientSpread".  Radial and focal gradients follow pixman's walker bit for bit; a LINEAR
                                            gradient with a spread other than pad is SWFR_ERR_NOT_IMPLEMENTED, "NotImplementedGradientSpread"
                                            (refused, never approximated) unless the handle has SWFR_FLAG_LINEAR_PIXMAN, which draws it as pixman does.  Ignored for solid and bitmap fills.  The field lies in what was
                                            the struct's tail padding: size and offsets are unchanged.  DESIGN.md, "Gradient spread modes" */
    uint8_t pad;                         /* bitmap: 1 = a padded ("clipped") fill, SWF fill types 0x41 / 0x43 -- the bitmap's Cairo pattern with
                                            cairo_pattern_set_extend(CAIRO_EXTEND_PAD): a sample outside the bitmap reads the nearest edge
                                            texel (the coordinates clamped per axis) and the fill is not cut to the bitmap's rectangle.
                                            0: `repeating` decides as before (EXTEND_REPEAT / EXTEND_NONE, the reference's behaviour), byte
                                            for byte.  pad = 1 together with repeating != 0, or pad > 1: SWFR_ERR_INVALID, "InvalidBitmapPad".
                                            Ignored for solid and gradient fills.  Offset 59, in the remaining tail padding: size (64) and
                                            every other offset are unchanged.  DESIGN.md, "Padded bitmap fills" */
    uint8_t filter;                      /* bitmap: the Cairo filter of the bitmap's surface pattern.  0 = CAIRO_FILTER_GOOD, what was always
                                            drawn, byte for byte (bilinear at 0.75 x and above, pixman's separable convolution below);
                                            `smoothed` is still ignored, as the reference ignores it.  1 = CAIRO_FILTER_NEAREST, an
                                            unsmoothed fill (SWF fill types 0x42 / 0x43): with f pixman's 16.16 position of the pixel centre,
                                            the ONE texel ((fx - 1) >> 16, (fy - 1) >> 16) -- a sample exactly on a texel edge reads the
                                            texel to the left of / above it -- at every scale (no convolution), the extend applied to that
                                            coordinate; an EXTEND_NONE fill is cut to the bitmap's rectangle padded by 0.004 source pixels
                                            and rounded to the nearest pixel edge on both axes.  Combines freely with `repeating` and `pad`.
                                            Above 1: SWFR_ERR_INVALID, "UnknownBitmapFilter".  Ignored for solid and gradient fills.  A
                                            decoder that wants Flash's result sets filter = smoothed ? 0 : 1.  Offset 60, in the remaining
                                            tail padding: size (64) and every other offset are unchanged.  DESIGN.md, "Unsmoothed bitmap
                                            fills" */
} swfr_fill_style;

typedef struct {
    uint32_t width, morph_width;         /* twips; caps/joins of the SWF style are dropped by the
                                            reference (decode-swf-shape.ts:144-149) */
    swfr_fill_style fill;
} swfr_line_style;

typedef struct {
    uint32_t n_fill; const swfr_fill_style *fill;
    uint32_t n_line; const swfr_line_style *line;
} swfr_styles;

enum { SWFR_RECORD_EDGE = 0, SWFR_RECORD_STYLE_CHANGE = 1 };

typedef struct {
    uint32_t type;                       /* SWFR_RECORD_* */
    /* edge */
    int32_t delta_x, delta_y;
    uint8_t has_control_delta; int32_t control_delta_x, control_delta_y;
    int32_t morph_delta_x, morph_delta_y;                              /* morph shapes */
    uint8_t has_morph_control_delta; int32_t morph_control_delta_x, morph_control_delta_y;
    /* style change */
    uint8_t has_move_to; int32_t move_to_x, move_to_y;
    uint8_t has_morph_move_to; int32_t morph_move_to_x, morph_move_to_y;
    uint8_t has_left_fill; uint32_t left_fill;
    uint8_t has_right_fill; uint32_t right_fill;
    uint8_t has_line_style; uint32_t line_style;
    const swfr_styles *new_styles;       /* NULL when absent */
} swfr_shape_record;

typedef struct {                         /* tags::DefineShape / tags::DefineMorphShape */
    uint32_t id;
    swfr_rect bounds, morph_bounds;
    swfr_styles initial_styles;
    uint32_t n_records; const swfr_shape_record *records;
} swfr_define_shape;

/* ---- stage ------------------------------------------------------------------------------- */
enum { SWFR_OBJECT_SHAPE = 0, SWFR_OBJECT_MORPH_SHAPE = 1, SWFR_OBJECT_CONTAINER = 2,
       SWFR_OBJECT_COLOR_TRANSFORM = 3   /* a container (matrix + children) whose `id` names a colour-transform slot (swfr_set_color_transform):
                                            the slot's value at the time of the render call applies to everything below it.  Beyond the
                                            reference, whose display objects carry a matrix and a ratio only */,
       /* 4 is not a display-object type: SWFR_ERR_INVALID, "UnexpectedDisplayObjectType" (as are 6, 7, 9, 10, 12, 14, 15, 17, 18, 20 and 22 and above) */
       SWFR_OBJECT_BLEND_MODE = 5,       /* a container (matrix + children) whose `id` is an SWF blend-mode number (SWFR_BLEND_*): every path
                                            drawn below it is composited, each on its own, with the mode's Cairo operator -- what
                                            CanvasRenderer would do if it set ctx.globalCompositeOperation before drawing the object.  It
                                            draws nothing itself; the innermost mode wins, an inner SWFR_BLEND_NORMAL restores OVER.  The
                                            paths are NOT composited as one layer: that is SWFR_OBJECT_LAYER.  DESIGN.md, "Blend modes" */
       SWFR_OBJECT_LAYER = 8             /* an isolated group: a container (matrix + children) whose children are drawn onto a transparent
                                            surface of the frame's size, which is then composited onto the parent as ONE layer with the
                                            operator of the SWF blend-mode number in `id` -- cairo_push_group; the children;
                                            cairo_pop_group_to_source; cairo_set_operator; cairo_paint.  0, 1, 2 (normal, layer): OVER;
                                            3..8, 13, 14: the mode's operator; 9..12: SWFR_ERR_NOT_IMPLEMENTED, "NotImplementedBlendMode"
                                            (11 and 12 are accepted on a handle with SWFR_FLAG_ALPHA_MODES: SWFR_BLEND_*, below);
                                            above 14: SWFR_ERR_INVALID.  A SWFR_OBJECT_BLEND_MODE in force around the layer still applies
                                            per path inside it, against the layer's own pixels.  Layers nest up to SWFR_MAX_LAYER_DEPTH
                                            deep: deeper is SWFR_ERR_CAPACITY, "LayerDepth".  (Masks: SWFR_OBJECT_MASKED_LAYER.)  A colour
                                            transform around a layer recolours the definitions below it; fading the layer as a whole
                                            is SWFR_OBJECT_FADED_LAYER.  DESIGN.md, "Isolated layers" */,
       SWFR_OBJECT_MASKED_LAYER = 11     /* a masked layer: a container (matrix + children) whose children[0] is the MASK subtree and whose
                                            children[1..] are the content.  Both are drawn as isolated groups that start clear --
                                            cairo_push_group; the content; content = cairo_pop_group; cairo_push_group; the mask; mask =
                                            cairo_pop_group; cairo_set_source(content); cairo_set_operator; cairo_mask(mask) -- and per
                                            pixel the parent's d becomes combine_op(mul_un8(C, Ma), d): C the content's premultiplied
                                            pixel, Ma the mask group's ALPHA (its colour channels play no part), mul_un8 per channel with
                                            0x80 rounding, combine_op the unmasked combiner of SWFR_OBJECT_LAYER.  `id` is an SWF
                                            blend-mode number, accepted exactly as SWFR_OBJECT_LAYER accepts it.  The object's matrix
                                            applies to both halves.  n_children == 0: SWFR_ERR_INVALID, "MaskedLayerWithoutMask".  A
                                            masked layer uses TWO levels of SWFR_MAX_LAYER_DEPTH.  Unlike a Flash clip-depth mask the
                                            mask's alpha counts and so do its strokes (geometry only: put the mask under a colour
                                            transform with alpha mult 0, add 255).  DESIGN.md, "Masked layers" */,
       /* 12 is not a display-object type */
       SWFR_OBJECT_FADED_LAYER = 13      /* a layer with an opacity: SWFR_OBJECT_LAYER whose composite is cairo_paint_with_alpha --
                                            cairo_push_group; the children; cairo_pop_group_to_source; cairo_set_operator;
                                            cairo_paint_with_alpha(opacity / 255.0) -- so that the children fade as ONE image: per pixel
                                            the parent's d becomes combine_op(mul_un8(g, opacity), d), g the group's premultiplied pixel,
                                            mul_un8 per channel, alpha included, with 0x80 rounding.  `id` is mode | opacity << 8: the
                                            mode an SWF blend-mode number, accepted exactly as SWFR_OBJECT_LAYER accepts it, the opacity
                                            0..255; id >= 0x10000: SWFR_ERR_INVALID.  Opacity 255 is SWFR_OBJECT_LAYER byte for byte,
                                            opacity 0 draws nothing.  One level of SWFR_MAX_LAYER_DEPTH; nests with the other two layer
                                            types.  DESIGN.md, "Layer opacity" */,
       /* 14 and 15 are not display-object types */
       SWFR_OBJECT_BLURRED_LAYER = 16    /* a blurred layer: a container (matrix + children) whose children are drawn onto a transparent
                                            surface of the frame's size, which is box-blurred and then composited onto the parent as ONE
                                            layer -- cairo_push_group; the children; cairo_pop_group; the blur on the group's surface;
                                            cairo_set_source; cairo_set_operator; cairo_paint.  `id` is mode | blur_x << 8 | blur_y << 16 |
                                            passes << 24: the mode an SWF blend-mode number, accepted exactly as SWFR_OBJECT_LAYER accepts
                                            it; blur_x, blur_y 0..255 the box widths in device pixels (0 and 1: that axis is left alone),
                                            not scaled by any matrix; passes 1..15 (0 or more: SWFR_ERR_INVALID, "InvalidBlur").  The blur
                                            (blur_x, blur_y, passes) is `passes` times a horizontal pass of width max(1, blur_x), then a
                                            vertical pass of width max(1, blur_y); one pass of width w is what pixman 0.40 computes for a
                                            PIXMAN_FILTER_CONVOLUTION of w equal taps (swfr_blur_bitmap).  What the children draw outside the
                                            frame is gone before the blur.  The children are built into a sub-frame of their own
                                            (swfr_built_layer) which swfr_render renders, captures and blurs on the device before the
                                            parent frame; in the parent the object is one SWFR_PATH_BOXES path over the whole frame with a
                                            nearest-filtered SWFR_STYLE_BITMAP style naming texture SWFR_BLUR_BASE + k.  A blurred layer
                                            below another: SWFR_ERR_NOT_IMPLEMENTED, "NestedBlur"; more than SWFR_MAX_BLUR_LAYERS in a
                                            frame: SWFR_ERR_CAPACITY, "BlurLayers".  The other layer types may sit inside and around it; the
                                            sub-frame counts its own SWFR_MAX_LAYER_DEPTH.  Only swfr_render draws it: swfr_render_batch,
                                            swfr_render_sequence and swfr_render_sequence_readback answer SWFR_ERR_NOT_IMPLEMENTED,
                                            "NotImplementedBlurRoute", a handle with band_count > 1 "NotImplementedBlurBands".
                                            DESIGN.md, "Blurred layers" */,
       /* 17 and 18 are not display-object types */
       SWFR_OBJECT_SHADOWED_LAYER = 19   /* a shadowed layer (drop shadow, glow): a container (matrix + children) whose children are drawn
                                            onto a transparent surface of the frame's size, as a blurred layer's are; the surface with its
                                            shadow (swfr_shadow, below: the group's alpha shifted, box-blurred, multiplied, tinted, and the
                                            group over it, cut out of it, or left out) is composited onto the parent as ONE layer.  `id` is
                                            mode | slot << 8: the mode an SWF blend-mode number, accepted exactly as SWFR_OBJECT_LAYER
                                            accepts it; the slot (< 65536) one set with swfr_set_shadow, whose value at the scene walk is
                                            the shadow -- an unset slot: SWFR_ERR_NOT_FOUND, "ShadowNotFound".  Built, numbered, limited and
                                            refused together with blurred layers: a sub-frame of its own (swfr_built_layer,
                                            swfr_built_layer_shadow), one box path in the parent naming texture SWFR_BLUR_BASE + k, at most
                                            SWFR_MAX_BLUR_LAYERS of both kinds in a frame ("BlurLayers"), neither kind below either
                                            ("NestedBlur"), drawn by swfr_render only ("NotImplementedBlurRoute", "NotImplementedBlurBands").
                                            DESIGN.md, "Shadowed layers" */,
       /* 20 is not a display-object type */
       SWFR_OBJECT_FILTERED_LAYER = 21   /* a layer with an ordered filter list: a container (matrix + children) whose children are drawn
                                            onto a transparent surface of the frame's size, as a blurred layer's are; the list's entries
                                            (swfr_filter, below: box blurs, shadows and convolutions, 1..SWFR_MAX_FILTERS of them) are applied to that
                                            surface one after the other, each to the result of the one before it -- a shadow later in the
                                            list shadows the earlier filters' output, earlier shadows included --, and the last result is
                                            composited onto the parent as ONE layer.  `id` is mode | slot << 8: the mode an SWF blend-mode
                                            number, accepted exactly as SWFR_OBJECT_LAYER accepts it; the slot (< 65536) one set with
                                            swfr_set_filters, whose list at the scene walk is the list, checked again there -- an unset
                                            slot: SWFR_ERR_NOT_FOUND, "FiltersNotFound".  A list of one entry is the blurred or shadowed
                                            layer of that entry, byte for byte.  Built, numbered, limited and refused together with
                                            blurred and shadowed layers: a sub-frame of its own (swfr_built_layer, swfr_built_layer_filters),
                                            one box path in the parent naming texture SWFR_BLUR_BASE + k, at most SWFR_MAX_BLUR_LAYERS of
                                            the three kinds in a frame whatever the lists' lengths ("BlurLayers"), none of the three below
                                            any of the three ("NestedBlur"), drawn by swfr_render only ("NotImplementedBlurRoute",
                                            "NotImplementedBlurBands").  DESIGN.md, "Filter lists" */ };
#define SWFR_MAX_LAYER_DEPTH 4
#define SWFR_MAX_BLUR_LAYERS 8           /* blurred, shadowed and filtered layers in one frame, together */
#define SWFR_BLUR_BASE 131072            /* swfr_style::bitmap of the k-th blurred layer of a frame: SWFR_BLUR_BASE + k */

/* SWF blend-mode numbers (PlaceObject3, swf-tree BlendMode).  0, 1: OVER.  3..8, 13, 14: the Cairo operator of the same name
   (CAIRO_OPERATOR_MULTIPLY, SCREEN, LIGHTEN, DARKEN, DIFFERENCE, ADD, OVERLAY, HARD_LIGHT).  SUBTRACT, INVERT, ALPHA, ERASE have no
   Cairo operator or act on a parent layer's alpha, and LAYER means nothing for a SWFR_OBJECT_BLEND_MODE (it is SWFR_OBJECT_LAYER's
   OVER): SWFR_ERR_NOT_IMPLEMENTED, "NotImplementedBlendMode".  Above 14: SWFR_ERR_INVALID.
   On a handle with SWFR_FLAG_ALPHA_MODES two of the four are accepted ("Erase and alpha modes"):
   ERASE (12) is CAIRO_OPERATOR_DEST_OUT, d' = mul_un8(d, 255 - sa) in every channel: as a SWFR_OBJECT_BLEND_MODE (per path) and as the
   mode of the three layer types (the group, masked or faded as ever, is the source of one DEST_OUT composite);
   ALPHA (11) is CAIRO_OPERATOR_DEST_IN, d' = mul_un8(d, sa): as the mode of the three layer types only.  Like canvas
   "destination-in" it is unbounded: the parent surface is cleared wherever the layer is transparent, outside the layer's own bounds
   too (Flash Player confines it to them).  As a SWFR_OBJECT_BLEND_MODE it stays "NotImplementedBlendMode": per path every single
   fill or stroke would clear the surface outside itself.  Neither mode needs a "layer" parent: outside any layer the surface is the
   frame.  SUBTRACT and INVERT stay refused. */
enum { SWFR_BLEND_NORMAL0 = 0, SWFR_BLEND_NORMAL = 1, SWFR_BLEND_LAYER = 2, SWFR_BLEND_MULTIPLY = 3, SWFR_BLEND_SCREEN = 4,
       SWFR_BLEND_LIGHTEN = 5, SWFR_BLEND_DARKEN = 6, SWFR_BLEND_DIFFERENCE = 7, SWFR_BLEND_ADD = 8, SWFR_BLEND_SUBTRACT = 9,
       SWFR_BLEND_INVERT = 10, SWFR_BLEND_ALPHA = 11, SWFR_BLEND_ERASE = 12, SWFR_BLEND_OVERLAY = 13, SWFR_BLEND_HARDLIGHT = 14 };

typedef struct swfr_display_object {
    uint32_t type;                       /* SWFR_OBJECT_* (ts/src/lib/display/display-object-type.ts) */
    uint32_t id;                         /* value returned by swfr_register_shape / swfr_register_morph_shape */
    uint8_t has_matrix; swfr_matrix matrix;
    double ratio;                        /* morph shapes: [0,1] (ts/src/lib/display/morph-shape.ts:9);
                                            Rust MorphRatio(u16) maps as ratio = v / 65535.0 */
    uint32_t n_children; const struct swfr_display_object *children;   /* containers */
} swfr_display_object;

typedef struct {
    uint32_t width, height;              /* carried for API parity; the frame size is the handle's */
    swfr_rgba8 background_color;         /* not painted by the reference (canvas-renderer.ts:72) */
    uint32_t n_children; const swfr_display_object *children;
} swfr_stage;

/* ---- colour transforms (swf-tree ColorTransformWithAlpha, PlaceObject2/3's CXFORMWITHALPHA) -------------------------------
   Channels r, g, b, a.  mult in Sfixed8P8 epsilons (256 = 1.0); all eight values in the int16 range.  One channel maps as
   c' = clamp(((c * mult) >> 8) + add, 0, 255) in int32 with an arithmetic shift; nested transforms apply innermost first, each one
   clamping.  What is transformed is the straight colour a definition holds: solid fill and line colours, gradient stops, both
   colours of a morph shape (the ratio interpolation comes after), and every straight texel of a bitmap fill as registered (before
   the putImageData premultiply and any filtering).  The stage background is not.  DESIGN.md, "Colour transforms". */
typedef struct { int32_t mult[4], add[4]; } swfr_color_transform;
/* Sets slot `slot` (< 65536) of the handle, or clears it (ct == NULL).  Out-of-range values: SWFR_ERR_INVALID.  A display object of
   type SWFR_OBJECT_COLOR_TRANSFORM naming an unset slot makes the render call fail with SWFR_ERR_NOT_FOUND ("ColorTransformNotFound"). */
int swfr_set_color_transform(swfr_renderer *r, uint32_t slot, const swfr_color_transform *ct);

/* ---- shadows (drop shadow and glow; DESIGN.md, "Shadowed layers") -----------------------------------------------------------
   The shadow of a group surface G (premultiplied, of the frame's size) as a libcairo 1.16 / pixman 0.40 call sequence, byte for byte:
     S   clear; cairo_set_source_rgba(0, 0, 0, 1); cairo_mask_surface(G, dx, dy):  S(x, y) = Ga(x - dx, y - dy) << 24, 0 where that
         pixel lies outside the frame -- dx, dy whole device pixels;
     S   box-blurred as swfr_blur_bitmap blurs (blur_x, blur_y, passes); the colour channels stay 0;
     T   clear; `strength` times CAIRO_OPERATOR_ADD paints S:  Ta = min(255, strength * Sa);
     Tc  clear; cairo_set_source_rgba(color / 255); cairo_mask_surface(T, 0, 0):  Tc = mul_un8(cp, Ta) in every channel, cp the colour's
         premultiplied pixel as Cairo makes it (each of a, r * a, g * a, b * a in doubles, * 65535 + 0.5 to 16 bits, >> 8);
     R   SWFR_SHADOW_HIDE_OBJECT: Tc.  SWFR_SHADOW_KNOCKOUT: CAIRO_OPERATOR_DEST_OUT paint of G, R = mul_un8(Tc, 255 - Ga).  Neither:
         OVER paint of G, R = G + mul_un8(Tc, 255 - Ga), saturating.  Both: invalid.
   An inner shadow (SWFR_SHADOW_INNER) is made of the inverse of the group's alpha and composited inside the group; S and R change,
   the blur, T and Tc do not:
     S'  clear; cairo_set_source_rgba(0, 0, 0, 1); cairo_paint; CAIRO_OPERATOR_DEST_OUT; cairo_mask_surface(G, dx, dy):
         S(x, y) = (255 - Ga(x - dx, y - dy)) << 24, and 255 << 24 where that pixel lies outside the frame (it counts as empty);
     R'  SWFR_SHADOW_INNER alone: CAIRO_OPERATOR_ATOP paint of Tc onto G, R = mul_un8(Tc, Ga) + mul_un8(G, 255 - Tca) per channel,
         saturating; R's alpha is G's.  With SWFR_SHADOW_KNOCKOUT: CAIRO_OPERATOR_DEST_IN paint of G onto Tc, R = mul_un8(Tc, Ga) --
         only the shadow, only inside the object.  With SWFR_SHADOW_HIDE_OBJECT: invalid -- inside the object "hide the object" and
         "knock out" are the same picture, and it is offered once, as the knockout.
   An inner glow is an inner shadow with dx = dy = 0.  The blur reads 0 beyond the frame, so an object that runs off the frame gets no
   inner shadow along the frame's edge (right for an object that continues there; a Flash bitmap ends at the object's bounds); an
   offset that shifts the whole group out of the frame gives a uniformly tinted object.
   A glow is a shadow with dx = dy = 0.  Not Flash Player's DropShadowFilter / GlowFilter: the box and the offset are whole device
   pixels that no matrix scales (a caller rounds distance * (cos, sin)(angle) itself), the strength is whole (Flash: 8.8 fixed), there
   is no quality beyond `passes`, the surface is cut to the frame before the shadow is made, an even box sits
   where pixman puts it, and a colour transform around the object recolours what is drawn inside, not the shadow.
   Ranges: blur_x, blur_y 0..255; passes 1..15; dx, dy -32768..32767; strength 1..255; flags 0, 1, 2, 8 or 10 (HIDE_OBJECT, KNOCKOUT, INNER,
   INNER | KNOCKOUT); anything else is SWFR_ERR_INVALID, "InvalidShadow".  Bit 2 (value 4) is skipped on purpose: flags 4 and 5 have been
   refused by name since shadows exist, the tests of the shadow and filter-list features hold them so, and they stay refused. */
#define SWFR_SHADOW_HIDE_OBJECT 1u
#define SWFR_SHADOW_KNOCKOUT 2u
#define SWFR_SHADOW_INNER 8u
typedef struct { uint32_t blur_x, blur_y, passes; int32_t dx, dy; swfr_rgba8 color; uint32_t strength, flags; } swfr_shadow;
/* Sets shadow slot `slot` (< 65536) of the handle, or clears it (shadow == NULL), as swfr_set_color_transform does for its slots.  A
   value out of range: SWFR_ERR_INVALID, "InvalidShadow".  SWFR_OBJECT_SHADOWED_LAYER names a slot. */
int swfr_set_shadow(swfr_renderer *r, uint32_t slot, const swfr_shadow *shadow);

/* ---- filter lists ("Filter lists") --------------------------------------------------------------------------------
   An ordered list of 1..SWFR_MAX_FILTERS filters of a group surface R_0 (premultiplied, of the frame's size), entry i made of R_(i-1):
     SWFR_FILTER_BLUR    R_i = R_(i-1) box-blurred as swfr_blur_bitmap blurs, on all four channels.  The entry uses shadow.blur_x,
                         shadow.blur_y (0..255) and shadow.passes (1..15); every other field of `shadow` must be zero.
     SWFR_FILTER_SHADOW  R_i = the final surface R of swfr_shadow, above, with G := R_(i-1): what is shadowed is the earlier filters'
                         output, earlier shadows included.  The entry's `shadow` is checked as swfr_set_shadow checks one.
     SWFR_FILTER_CONVOLUTION
                         R_i = R_(i-1) convolved with the kernel (swfr_kernel, below) of the slot that shadow.blur_x names (0..65535),
                         as swfr_convolve_bitmap convolves, on all four channels.  Every other field of `shadow` must be zero.  The
                         kernel is the slot's value at the scene walk, like a shadowed layer's shadow: an unset slot there is
                         SWFR_ERR_NOT_FOUND, "KernelNotFound" (swfr_set_filters does not look at the slot).
   Not Flash Player's filter list: these three kinds only (no bevel, gradient glow or colour matrix), four
   entries at most, and every caveat of swfr_blur_bitmap's box, of swfr_shadow and of swfr_kernel holds for each entry.
   An unknown kind or a value out of range: SWFR_ERR_INVALID, "InvalidFilter".  Kinds 2 and 3 are skipped on purpose: they, 255 and
   2^32 - 1 have been refused by name since filter lists exist, the tests of that feature hold them so, and they stay refused. */
#define SWFR_MAX_FILTERS 4
enum { SWFR_FILTER_BLUR = 0, SWFR_FILTER_SHADOW = 1, SWFR_FILTER_CONVOLUTION = 4 };
typedef struct { uint32_t kind; swfr_shadow shadow; } swfr_filter;
/* Sets filter-list slot `slot` (< 65536) of the handle to the `count` entries at `filters`, or clears it (filters == NULL or count == 0),
   as swfr_set_shadow does for its slots.  A slot above 65535, an unknown kind or a value out of range: SWFR_ERR_INVALID,
   "InvalidFilter"; count > SWFR_MAX_FILTERS: SWFR_ERR_CAPACITY, "FilterListLength".  A refused call leaves the slot as it was.
   SWFR_OBJECT_FILTERED_LAYER names a slot. */
int swfr_set_filters(swfr_renderer *r, uint32_t slot, const swfr_filter *filters, uint32_t count);

/* ---- convolution kernels ("Convolution filters") -------------------------------------------------------------------
   A kernel of width x height taps (1..SWFR_MAX_KERNEL_DIM each way) in row-major order, each a signed 16.16 number.  For every pixel
   (x, y) of a premultiplied image and every channel c, alpha included and treated like the colours:
     S = sum_j sum_i taps[j * width + i] * c(x - width / 2 + i, y - height / 2 + j) + 0x8000
     out = S < 0 ? 255 : min(255, S >> 16)
   -- integer divisions, a tap outside the image reading 0: what pixman 0.40 computes for PIXMAN_FILTER_CONVOLUTION with these taps
   under PIXMAN_OP_SRC from an image of EXTEND_NONE, byte for byte.  A NEGATIVE SUM GIVES 255, NOT 0: pixman 0.40 keeps the sums in
   unsigned integers (pixman-bits-image.c, reduce_32), so a negative one is a huge one and clips at the top.  A sharpen, emboss or edge
   kernel therefore turns the pixels it would darken below zero fully bright, alpha included; this library follows libpixman, the
   yardstick it is held against, and does not mend it.  The window sits where a
   box of swfr_blur_bitmap sits: an even size reaches one pixel further left and up.  The sum of the taps' absolute values is at most
   8 388 607 (below 128.0): a kernel beyond that is refused, never wrapped.  All taps zero is legal (a clear surface); the 1 x 1 kernel
   {65536} is the identity.  Negative taps make pixels whose colour exceeds their alpha; what follows (later entries, the composite)
   treats them with the saturating arithmetic libcairo treats them with.
   Not Flash Player's ConvolutionFilter: no bias, no preserveAlpha (alpha is convolved like the colours, on premultiplied pixels), no
   clamp / color (outside the frame reads clear); dimensions up to 7; the taps are in device pixels, which no matrix scales; the
   surface is cut to the frame first; the caller folds the divisor into the taps.
   A dimension of 0 or above 7, or a sum beyond the bound: SWFR_ERR_INVALID, "InvalidKernel". */
#define SWFR_MAX_KERNEL_DIM 7
typedef struct { uint32_t width, height; int32_t taps[49]; } swfr_kernel;
/* Sets kernel slot `slot` (< 65536) of the handle, or clears it (kernel == NULL), as swfr_set_shadow does for its slots.  A refused call
   leaves the slot as it was.  A filter entry of kind SWFR_FILTER_CONVOLUTION names a slot. */
int swfr_set_kernel(swfr_renderer *r, uint32_t slot, const swfr_kernel *kernel);

/* ---- configuration ------------------------------------------------------------------------ */
#define SWFR_DEVICE_HOST_ONLY (-1)       /* decode + geometry only; swfr_render fails with NO_DEVICE */
#define SWFR_FLAG_EVEN_ODD 1u            /* fill rule override (the reference always uses nonzero) */
#define SWFR_FLAG_BANDS_CONTIGUOUS 2u    /* multi-GPU: this handle's tile-rows are one contiguous block, see band_index below */
#define SWFR_FLAG_ANTIALIAS_NONE 4u      /* aliased edges: cairo_set_antialias(cr, CAIRO_ANTIALIAS_NONE), node-canvas's
                                            ctx.antialias = 'none' (the reference always antialiases): polygons are sampled at pixel
                                            centres, rectilinear paths rounded to whole pixels; every render route honours it */
#define SWFR_FLAG_LINEAR_PIXMAN 8u       /* a SWFR_FILL_LINEAR_GRADIENT becomes a SWFR_STYLE_LINEAR_PIXMAN style -- libcairo's bytes, every
                                            spread -- instead of the float64 model (within +-1 of Cairo, pad only).  Together with
                                            SWFR_FLAG_ANTIALIAS_NONE: swfr_create fails with SWFR_ERR_NOT_IMPLEMENTED
                                            ("NotImplementedAliasedPixmanLinear", readable with swfr_last_error(NULL) on the same thread) */
#define SWFR_FLAG_ALPHA_MODES 16u        /* the blend modes ERASE (12) and ALPHA (11) are accepted (SWFR_BLEND_*, above) and so are the path
                                            operators SWFR_OP_ERASE and SWFR_OP_ALPHA at swfr_upload_edges.  Without the flag every
                                            refusal and every byte is what it was */

typedef struct {
    int32_t device;                      /* HIP device ordinal, or SWFR_DEVICE_HOST_ONLY */
    uint32_t flags;
    uint32_t band_index, band_count;     /* multi-GPU: this handle rasterizes the tile-rows (16 pixel rows each) t with
                                            t % band_count == band_index (0,0|1 = all), or, with SWFR_FLAG_BANDS_CONTIGUOUS,
                                            the block [band_index * n, (band_index + 1) * n), n = ceil(tile-rows / band_count):
                                            a rank's part of the frame is then one contiguous range of rows, which a gather can
                                            deposit in the assembled image without a copy */
} swfr_config;

/* ---- lifecycle / assets / render ----------------------------------------------------------- */
int  swfr_create(uint32_t width, uint32_t height, const swfr_config *cfg, swfr_renderer **out);
void swfr_destroy(swfr_renderer *r);
const char *swfr_last_error(const swfr_renderer *r);   /* r == NULL: "null handle" -- or, after a swfr_create on this thread refused a combination
                                                          of flags (SWFR_FLAG_LINEAR_PIXMAN with SWFR_FLAG_ANTIALIAS_NONE), that refusal's name, until the
                                                          thread's next swfr_create */
uint32_t swfr_abi_version(void);

int  swfr_register_shape(swfr_renderer *r, const swfr_define_shape *tag, uint32_t *out_id);
int  swfr_register_morph_shape(swfr_renderer *r, const swfr_define_shape *tag, uint32_t *out_id);
int  swfr_register_bitmap(swfr_renderer *r, uint32_t id, uint32_t width, uint32_t height,
                          const uint8_t *rgba_straight, size_t stride);
/* Renderer.addBitmap(tag) with the tag's own bytes (ts/src/lib/renderers/node-canvas-bitmap-service.ts:14-37): media type
   "image/x-swf-bmp" is decoded by the library (decodeXSwfBmpSync, ts/src/lib/decode-x-swf-bmp.ts:9-41: format 3, zlib colour-mapped,
   rows padded to 4 bytes, opaque palette, an index past the palette is opaque black) and registered as by swfr_register_bitmap;
   any other media type, or another format id, is SWFR_ERR_NOT_IMPLEMENTED like the reference's "NotImplemented: Support for ...
   images" / "UnsupportedXSwfBmpFormatId"; a damaged stream is SWFR_ERR_INVALID. */
int  swfr_register_bitmap_tag(swfr_renderer *r, uint32_t id, const char *media_type, const uint8_t *data, size_t len);
/* The decoder alone (no handle, no device): dimensions, and -- when rgba is not NULL -- straight RGBA8 with tight rows into the
   caller's buffer of rgba_cap bytes (SWFR_ERR_CAPACITY when it is too small; call with NULL first to size it). */
int  swfr_decode_x_swf_bmp(const uint8_t *data, size_t len, uint32_t *width, uint32_t *height, uint8_t *rgba, size_t rgba_cap);
int  swfr_render(swfr_renderer *r, const swfr_stage *stage);               /* blocking */
/* The last rendered frame becomes registered bitmap `bitmap_id` (< 65536), of the frame's size: its premultiplied pixels, device to
   device, no host copy.  Blocking; queued on the handle's stream behind everything pending on every frame set.  No frame yet:
   SWFR_ERR_INVALID; a host-only handle: SWFR_ERR_NO_DEVICE; a handle with band_count > 1, which holds only its own rows:
   SWFR_ERR_NOT_IMPLEMENTED, "NotImplementedBlurBands".  A captured bitmap has no straight texels: a colour transform over a fill that
   samples it is refused with SWFR_ERR_NOT_IMPLEMENTED, "NotImplementedCapturedBitmapTransform". */
int  swfr_capture_bitmap(swfr_renderer *r, uint32_t bitmap_id);
/* Registered bitmap `bitmap_id` box-blurred in place on the device (ping-pong with a scratch texture the handle keeps): `passes`
   (1..15) times a horizontal pass of box width max(1, blur_x), then a vertical pass of width max(1, blur_y); blur_x, blur_y 0..255;
   anything else SWFR_ERR_INVALID, "InvalidBlur"; an unknown id SWFR_ERR_NOT_FOUND.  One pass of width w >= 2 over the premultiplied
   ARGB texels, per channel, alpha included: out = min(255, (f * S + 0x8000) >> 16) with f = (65536 + w / 2) / w and S the sum over
   the window [x - w / 2, x - w / 2 + w - 1], texels outside the image reading 0 -- pixman 0.40's PIXMAN_FILTER_CONVOLUTION with w
   equal taps, byte for byte; w = 1 is the identity.  The bitmap's generation is bumped and it counts as captured from then on.
   Blocking, ordered like swfr_capture_bitmap. */
int  swfr_blur_bitmap(swfr_renderer *r, uint32_t bitmap_id, uint32_t blur_x, uint32_t blur_y, uint32_t passes);
/* Registered bitmap `src_id` plays the group G of a shadow (swfr_shadow, above); the final surface R becomes registered bitmap `dst_id`
   (< 65536; it may be src_id), of the same size: its generation is bumped and it counts as captured.  The alpha pass, the box passes
   and the finish pass run on the device (scratch textures the handle keeps).  `shadow` out of range: SWFR_ERR_INVALID,
   "InvalidShadow"; an unknown src_id: SWFR_ERR_NOT_FOUND.  Blocking, ordered like swfr_blur_bitmap. */
int  swfr_shadow_bitmap(swfr_renderer *r, uint32_t dst_id, uint32_t src_id, const swfr_shadow *shadow);
/* Registered bitmap `bitmap_id` convolved with `kernel` (swfr_kernel, above) on the device: one out-of-place pass over the premultiplied
   ARGB texels into a scratch texture the handle keeps, and the result back in the bitmap's own texture.  `kernel` NULL or out of range:
   SWFR_ERR_INVALID, "InvalidKernel"; a host-only handle: SWFR_ERR_NO_DEVICE; an unknown id: SWFR_ERR_NOT_FOUND.  The bitmap's
   generation is bumped and it counts as captured from then on.  Blocking, ordered like swfr_blur_bitmap. */
int  swfr_convolve_bitmap(swfr_renderer *r, uint32_t bitmap_id, const swfr_kernel *kernel);
int  swfr_read_image(swfr_renderer *r, uint8_t *dst, size_t dst_stride, int premultiplied);
/* Mapped read-back in two halves (HeadlessGfxRenderer::get_image maps its staging buffer the same way:
   rs/src/headless_renderer.rs:725-868): _async queues the device-to-host copy of the last frame into the handle's PINNED staging
   buffer behind the frame's kernels and returns; _wait blocks until it has arrived and hands out the staging buffer itself
   (width*4-byte rows, valid until the next read-back or swfr_destroy) -- no second copy on the host.  One read-back in flight per
   handle; ANY render call (swfr_render, swfr_render_resident(_async / _to), swfr_render_batch) may be issued before _wait: the
   host build overlaps the copy, and the streams of the handle's other frame sets are made to wait for the copy on the device before
   a frame is rasterized, so the image read back is never torn. */
int  swfr_read_image_async(swfr_renderer *r, int premultiplied);
int  swfr_read_image_wait(swfr_renderer *r, const uint8_t **data, size_t *stride);
/* render + mapped read-back of every frame, timed below the ABI (the reference's test loop: render, get_image). */
int  swfr_render_sequence_readback(swfr_renderer *r, const swfr_stage *stages, uint32_t n_stages, uint32_t repeat, int premultiplied,
                                   int overlap, double *seconds, uint64_t *checksum);

/* ---- low-level entry: the hot path proper (edge list -> RGBA8 in HBM) ---------------------- */
/* One edge of a flattened, limit-clipped polygon in 24.8 device coordinates: the line
   (x1,y1)-(x2,y2) with y1 < y2 is active for y in [top,bottom), y1 <= top < bottom <= y2 (an edge
   with top >= bottom is never active; any other edge active outside its own line is refused with
   SWFR_ERR_INVALID); dir is the winding direction.
   `reserved` is the index of the owning path (the device bins edges by it): swfr_build_frame fills
   it in, swfr_upload_edges / swfr_render_edges overwrite it from the paths' edge ranges. */
typedef struct { int32_t x1, y1, x2, y2, top, bottom, dir, reserved; } swfr_edge;

enum { SWFR_PATH_TOR = 0,   /* general polygon: Cairo "tor" 15x256 scan conversion */
       SWFR_PATH_BOXES = 1, /* rectilinear: `edges` hold disjoint boxes (x1,y1)-(x2,y2) */
       /* the two markers of an isolated group (SWFR_OBJECT_LAYER): the paths between them are drawn onto a transparent surface, which
          GROUP_END composites onto what was there at GROUP_BEGIN.  Both have n_edges 0 and the same rectangle: the union of the
          rectangles of the paths between them (those lie inside it).  BEGIN's `lerp` is 0; END's holds the composite's operator in bits
          8..15, 0 in bits 0..7 and 16..23, and in bits 24..31 the group's FADE, 255 - opacity (0: a plain group): the group's pixels
          are multiplied by the opacity (mul_un8 per channel, alpha included) before they are composited, SWFR_OBJECT_FADED_LAYER.  A
          fade on any other path, or on the END of a group that holds a GROUP_MASK (Cairo has no single call for a masked and faded
          composite: nest the two), is SWFR_ERR_INVALID.  Markers are balanced and nest at most SWFR_MAX_LAYER_DEPTH deep; their `style` is ignored.  Inside a
          group "the surface" of the lerp rule is the group's: its first paint is a SOURCE lerp.  SWFR_ERR_INVALID at upload otherwise */
       SWFR_PATH_GROUP_BEGIN = 2, SWFR_PATH_GROUP_END = 3,
       /* the third marker, of a masked group (SWFR_OBJECT_MASKED_LAYER): BEGIN; content paths; MASK; mask paths; END(operator).  The
          paths behind MASK are drawn onto a second transparent surface; END multiplies the content's pixels by that surface's alpha
          (mul_un8 per channel) and composites the product as GROUP_END does.  n_edges 0, lerp 0, the rectangle of its BEGIN and END
          (the union of all member rectangles, content and mask); at most one MASK per group, and none outside a group; a masked group
          counts two levels of SWFR_MAX_LAYER_DEPTH; groups nest inside either half.  SWFR_ERR_INVALID at upload otherwise */
       SWFR_PATH_GROUP_MASK = 4 };

typedef struct {
    uint32_t first_edge, n_edges;
    uint32_t kind;                       /* SWFR_PATH_* */
    uint32_t fill_rule;                  /* 0 nonzero, 1 even-odd */
    uint32_t style;                      /* index into styles */
    uint32_t lerp;                       /* bits 0..7: 1: SOURCE-lerp blend (opaque source or clear surface), 0: OVER.  With a bitmap or
                                            gradient style 1 means mul_un8(source pixel, coverage) with the destination ignored, and
                                            is defined only where the surface (the frame's, or inside a group the group's) is
                                            still clear under the path's rectangle: swfr_build_frame sets it while the surface is clear;
                                            bits 8..15: operator (SWFR_OP_*), 0: what bits 0..7 say.  An operator needs lerp bits 0
                                            (SWFR_ERR_INVALID at upload otherwise); the rest of the word must be 0 */
    int32_t x_min, y_min, x_max, y_max;  /* pixel rectangle of the converter (polygon extents ∩ frame) */
} swfr_path;

/* The operator of a path (swfr_path::lerp >> 8): pixman's unified combiner of that name applied to mul_un8(source pixel, coverage).
   Of a SWFR_PATH_GROUP_END: the same combiner applied to the group's pixel itself (no coverage). */
enum { SWFR_OP_OVER = 0, SWFR_OP_MULTIPLY = 1, SWFR_OP_SCREEN = 2, SWFR_OP_LIGHTEN = 3, SWFR_OP_DARKEN = 4, SWFR_OP_DIFFERENCE = 5,
       SWFR_OP_ADD = 6, SWFR_OP_OVERLAY = 7, SWFR_OP_HARDLIGHT = 8,
       /* on a handle with SWFR_FLAG_ALPHA_MODES only (without it: SWFR_ERR_INVALID as every value above 8).  With s the source as above
          and sa its alpha byte, per channel, alpha included, pixman's 0x80 rounding:
          ERASE, CAIRO_OPERATOR_DEST_OUT: d' = mul_un8(d, 255 - sa).  On an ordinary path (lerp bits 0) and on a GROUP_END.
          ALPHA, CAIRO_OPERATOR_DEST_IN: d' = mul_un8(d, sa).  On a GROUP_END only (an ordinary path: SWFR_ERR_INVALID).  The operator
          is unbounded -- where the group is transparent the parent surface becomes clear -- so an ALPHA GROUP_END and its BEGIN (and
          MASK) must carry a rectangle that contains the rectangle of every path since the enclosing surface began (the enclosing
          GROUP_BEGIN, or the frame's start): outside it the parent is clear anyway.  SWFR_ERR_INVALID otherwise */
       SWFR_OP_ERASE = 9, SWFR_OP_ALPHA = 10 };

enum { SWFR_STYLE_SOLID = 0, SWFR_STYLE_RADIAL = 1, SWFR_STYLE_LINEAR = 2, SWFR_STYLE_BITMAP = 3,
       SWFR_STYLE_LINEAR_PIXMAN = 4 };   /* 4: the linear gradient c0 -> c1 evaluated as pixman 0.40 does (linear_get_scanline), piece by
                                            piece as cairo 1.16 composites the shape -- bit-exact, with extend 0 pad, 1 repeat, 2 reflect.
                                            One path per style; c0 == c1 is SWFR_ERR_INVALID; a line other than a SWF fill's (-16384, 0)-(16384, 0) is
                                            SWFR_ERR_NOT_IMPLEMENTED, "NotImplementedLinearLine" (only that line has been held against libcairo); on a handle with SWFR_FLAG_ANTIALIAS_NONE
                                            SWFR_ERR_NOT_IMPLEMENTED, "NotImplementedAliasedPixmanLinear"; a rectilinear path of several
                                            boxes, or one box off the pixel grid wider than 256 px, "NotImplementedLinearPieces"; a position
                                            that moves by less than one 16.16 unit per pixel row without standing still,
                                            "NotImplementedLinearRowStep"; a rectangle that leaves pixman's 16.16 range SWFR_ERR_CAPACITY,
                                            "LinearGradientOutOfRange".  2 stays the float64 model.  DESIGN.md, "Pixman-exact linear gradients" */
#define SWFR_MAX_STOPS 16

typedef struct {
    uint32_t kind;                       /* SWFR_STYLE_* */
    uint32_t pixel;                      /* solid: premultiplied 0xAARRGGBB */
    double inv[6];                       /* device -> pattern space (xx, yx, xy, yy, x0, y0): Cairo's pattern matrix.  A bitmap
                                            style belongs to one drawing operation: pixman's 16.16 transform is anchored at the
                                            centre of the operation's pixel rectangle, so paths sharing it must share x_min..y_max */
    double c0x, c0y, r0, c1x, c1y, r1;   /* radial (linear: c0 -> c1) */
    uint32_t n_stops;
    float stop_offset[SWFR_MAX_STOPS];
    float stop_rgba[SWFR_MAX_STOPS][4];  /* straight, 0..1 */
    uint32_t bitmap;                     /* registered bitmap id; 65536 + k: texture k of the colour-transformed bitmaps of the frame the
                                            handle's last scene walk built (swfr_build_frame), valid on that handle until its next walk;
                                            131072 + k (SWFR_BLUR_BASE): the texture of the frame's k-th blurred or shadowed layer, which only swfr_render
                                            makes -- at swfr_upload_edges SWFR_ERR_NOT_FOUND */
    uint32_t extend;                     /* bitmap: 0 none, 1 repeat, 2 pad (CAIRO_EXTEND_PAD: swfr_fill_style::pad).  Radial / linear: 0 pad, 1 repeat, 2 reflect (cairo_pattern_set_extend);
                                            any other value on a gradient style is SWFR_ERR_INVALID at upload, and 1 or 2 on a LINEAR
                                            style SWFR_ERR_NOT_IMPLEMENTED, "NotImplementedGradientSpread" (a LINEAR_PIXMAN style takes all three) */
    uint32_t filter;                     /* bitmap: 0 CAIRO_FILTER_GOOD, 1 CAIRO_FILTER_NEAREST (swfr_fill_style::filter); any other value on a
                                            bitmap style is SWFR_ERR_INVALID at upload.  Ignored for every other kind.  Offset 436, in what
                                            was the struct's tail padding: the size (440) and every other offset are unchanged */
} swfr_style;

/* Upload a scene (kept resident in HBM), then rasterize it.  swfr_render_edges = upload + render. */
int  swfr_upload_edges(swfr_renderer *r, const swfr_edge *edges, size_t n_edges,
                       const swfr_path *paths, size_t n_paths,
                       const swfr_style *styles, size_t n_styles);
int  swfr_render_resident(swfr_renderer *r, uint32_t frames);              /* blocking; frames >= 1 */
/* Measurement entry: the resident scene as `frames_per_launch` (1..64) frames per kernel launch, every frame with its own
   kernel-written buffers and framebuffer, `launches` launches back to back (after one warm-up launch); *total_ms = HIP-event time of
   the `launches` launches.  The last frame is readable with swfr_read_image.  The saturated-GPU figure of bench.py.  The handle keeps
   the frames_per_launch framebuffers and work buffers (grow-only, like the frame sets': 64 x 33 MB at 4K) until swfr_destroy. */
int  swfr_render_resident_batched(swfr_renderer *r, uint32_t frames_per_launch, uint32_t launches, float *total_ms);
int  swfr_render_edges(swfr_renderer *r, const swfr_edge *edges, size_t n_edges,
                       const swfr_path *paths, size_t n_paths,
                       const swfr_style *styles, size_t n_styles);

/* Host half of swfr_render without the device: builds the frame's edge list exactly as
   swfr_render would upload it.  Arrays are owned by the handle until the next call. */
int  swfr_build_frame(swfr_renderer *r, const swfr_stage *stage,
                      const swfr_edge **edges, size_t *n_edges,
                      const swfr_path **paths, size_t *n_paths,
                      const swfr_style **styles, size_t *n_styles);

/* The sub-frames of the blurred, shadowed and filtered layers (SWFR_OBJECT_BLURRED_LAYER, _SHADOWED_LAYER, _FILTERED_LAYER) of the frame
   the handle's last scene walk built: how many, and the k-th one's arrays -- what swfr_render renders, captures and filters into texture
   SWFR_BLUR_BASE + k before the parent frame -- with its blur: a shadowed layer's shadow's box, a filtered layer's first entry's box ((0, 0, 1) where
   that entry is a convolution).
   Owned by the handle until its next walk; any out-parameter may be NULL.  k out of range: SWFR_ERR_NOT_FOUND. */
uint32_t swfr_built_layers(const swfr_renderer *r);
int  swfr_built_layer(swfr_renderer *r, uint32_t k,
                      const swfr_edge **edges, size_t *n_edges,
                      const swfr_path **paths, size_t *n_paths,
                      const swfr_style **styles, size_t *n_styles,
                      uint32_t *blur_x, uint32_t *blur_y, uint32_t *passes);
/* Whether the k-th sub-frame is a shadowed layer's (SWFR_OBJECT_SHADOWED_LAYER) and, if so, its shadow as the scene walk read it from
   the slot; swfr_built_layer reports that shadow's box.  A filtered layer's sub-frame (SWFR_OBJECT_FILTERED_LAYER) answers
   has_shadow = 0, whatever its list holds: swfr_built_layer_filters reports lists.  Either out-parameter may be NULL.  k out of range:
   SWFR_ERR_NOT_FOUND. */
int  swfr_built_layer_shadow(swfr_renderer *r, uint32_t k, int *has_shadow, swfr_shadow *out);
/* The filter list of the k-th sub-frame as the scene walk read it: `count` entries (1..SWFR_MAX_FILTERS) at `out`, which has room for
   SWFR_MAX_FILTERS.  A blurred layer's sub-frame reports its one blur entry, a shadowed layer's its one shadow entry.  Either
   out-parameter may be NULL.  k out of range: SWFR_ERR_NOT_FOUND. */
int  swfr_built_layer_filters(swfr_renderer *r, uint32_t k, uint32_t *count, swfr_filter *out);
/* The kernel the scene walk read for entry `entry` of the k-th sub-frame's filter list (swfr_built_layer_filters reports the entry
   itself as it was set: its kind and its slot).  k or entry out of range, or an entry that is no convolution: SWFR_ERR_NOT_FOUND.  `out`
   may be NULL. */
int  swfr_built_layer_kernel(swfr_renderer *r, uint32_t k, uint32_t entry, swfr_kernel *out);

/* Decoded paths of a registered (morph) shape as JSON text in the format of the reference's
   decode goldens (tests/<set>/<name>/shape.ts.json).  String owned by the handle. */
int  swfr_shape_json(swfr_renderer *r, uint32_t id, int morph, const char **json);

/* A batch of different frames in one call (the reference renders its 256 morph ratios by calling render 256 times,
   ts/src/test/node-canvas-renderer.spec.ts:86-113; rs/src/lib.rs:116-130).  With a device destination the frames are rendered
   in groups of up to SWFR_BATCH_FRAMES (default 64) by ONE launch per kernel and group, two groups alternating so that the host
   builds one while the GPU renders the other; frame i lands, premultiplied RGBA8 with tight rows, at device_dst + i * frame_stride
   (DEVICE memory, e.g. a torch tensor; both multiples of 4 bytes, else SWFR_ERR_INVALID "MisalignedTarget", see swfr_set_targets).  With device_dst == NULL the frames are rendered one after the other and only the last is
   kept for swfr_read_image.  Blocking: returns when every frame is finished.
   A refused frame (e.g. SWFR_ERR_NOT_FOUND for an unknown shape or bitmap) ends the batch with its error code, returned only after
   everything the call queued has finished: no frame is still being written.  The frames before it are complete, except that with
   a device destination the frames of the refused frame's own group (launched together) are not written either; no later slot is
   written.  The handle renders correctly afterwards; swfr_read_image returns SWFR_ERR_INVALID until the next frame is rendered. */
int  swfr_render_batch(swfr_renderer *r, const swfr_stage *stages, uint32_t n_stages, void *device_dst, size_t frame_stride);

/* Timing of the last swfr_render / swfr_render_resident, from HIP events on the handle's stream. */
typedef struct {
    float total_ms;                      /* first kernel start -> last kernel end, all frames */
    float setup_ms, rows_ms, tiles_ms;   /* per-kernel sums over the timed_frames frames that carried events */
    uint32_t frames;
    uint64_t n_edges, n_paths, n_row_tasks, n_records;
    uint32_t timed_frames;               /* frames / SWFR_EVENT_STRIDE (default 16) */
} swfr_timing;
int  swfr_last_timing(swfr_renderer *r, swfr_timing *out);

/* Where the time of the last swfr_render went (the reference's calling pattern: one blocking call per frame). */
typedef struct {
    double build_ms;                     /* host: Stage -> edge list (scene walk, flattening, stroking, clipping) */
    double upload_host_ms;               /* host: staging copy + table layout (prefix sums over the paths); for a frame with blurred
                                            layers also everything done for their sub-frames before the parent is uploaded -- each one
                                            uploaded, rendered, captured, blurred and waited for (device time included) */
    double h2d_ms;                       /* the scene's one host-to-device copy (HIP events) */
    double device_ms;                    /* first kernel start -> last kernel end (HIP events) */
    double total_ms;                     /* wall clock of the whole call, synchronisation included */
    uint64_t h2d_bytes;
} swfr_path_timing;
int  swfr_last_path_timing(swfr_renderer *r, swfr_path_timing *out);

/* What the row kernels met since the handle was created (summed over every frame whose counters came back): rows the fast kernel
   left to the general ones, rows that needed the replay of Cairo's edge-list order for coincident edges, and how often a capacity
   limit of that replay was reached -- each such frame was refused with SWFR_ERR_CAPACITY, never rendered approximately. */
typedef struct swfr_stats {
    uint64_t frames;                     /* frames whose counters were read back */
    uint64_t queued_rows;                /* (path, pixel row) pairs left to k2_rows_slow (coincident edges or > 8 active edges) */
    uint64_t crowded_rows;               /* ... of which handed on to k2_rows_huge (> 64 active edges) */
    uint64_t tie_rows;                   /* rows whose edge order came from the list-order replay */
    uint64_t pairtest_limit;             /* frames refused: crossing test over more than 2^21 edge pairs */
    uint64_t start_group_limit;          /* frames refused: more than 8192 edges of a path start at one sample row / are active in a row */
    uint64_t history_limit;              /* frames refused: order of two older coincident edges needs history deeper than two levels */
    uint64_t reserved;
} swfr_stats;
int  swfr_get_stats(swfr_renderer *r, swfr_stats *out);

/* The reference's animation loop in one call: for (rep < repeat) for (i < n_stages) swfr_render(stages[i]) -- every frame built,
   uploaded, binned, rasterized and waited for exactly as by swfr_render -- timed on the host side of the C-ABI.  `seconds`
   receives the wall clock of the loop; `sum` (optional) the per-stage times added up. */
int  swfr_render_sequence(swfr_renderer *r, const swfr_stage *stages, uint32_t n_stages, uint32_t repeat, double *seconds,
                          swfr_path_timing *sum);

/* Multi-GPU: copy this handle's band slab (its tile-rows, packed in order) into a caller-owned
   DEVICE buffer (e.g. a torch tensor's data_ptr) so that the caller can gather it with RCCL. */
size_t swfr_band_slab_bytes(const swfr_renderer *r);
int  swfr_copy_band_slab(swfr_renderer *r, void *device_dst);

/* Multi-GPU / pipelined use.  swfr_set_targets: the frames of the resident scene are rendered straight into caller-owned DEVICE
   buffers (width*height*4 bytes each, premultiplied RGBA8, tight rows; e.g. torch tensors) -- frame set k of the handle (there are
   SWFR_FRAMES_IN_FLIGHT of them, rotating) writes targets[k]; takes effect with the next swfr_upload_edges.  A handle that owns only
   some tile-rows writes only those rows.  swfr_render_resident_async queues one frame on the next frame set without waiting and
   reports which set (and so which target and which stream) it used; swfr_stream_handle gives that set's hipStream_t so that the
   caller's own streams can be ordered behind / before it with events; swfr_wait blocks until everything queued has finished and
   reports the kernels' error state like swfr_render_resident does.
   Alignment: every target, block target and batch destination is written as 32-bit words, so its address -- and the frame_stride
   of swfr_render_batch -- must be a multiple of 4 bytes; one that is not is refused with SWFR_ERR_INVALID and the message
   "MisalignedTarget" before anything is launched, and the handle keeps the targets it had.  Nothing more is asked: a target that
   is only 4-, 8- or 12-byte aligned is rendered into with narrower stores, to the same bytes. */
int  swfr_set_targets(swfr_renderer *r, void *const *device_targets, uint32_t n_targets);
int  swfr_render_resident_async(swfr_renderer *r, uint32_t *out_set);
/* The same, with THIS frame's pixels going to block_target: a device buffer that holds only the handle's own block of tile-rows
   (a handle with SWFR_FLAG_BANDS_CONTIGUOUS: rows_of_the_block * width * 4 bytes, the block's first pixel row first).  Any number of
   such buffers may be in flight -- they are not tied to the handle's frame sets -- which is what an exchange of SEVERAL frames at once
   needs (frame f assembled on rank f mod N, the N frames' blocks sent in one grouped all-to-all: DESIGN.md, multi-GPU). */
int  swfr_render_resident_async_to(swfr_renderer *r, void *block_target, uint32_t *out_set);
/* n_frames such frames (<= 64), one per block target, queued in one call; *sets_used: bit k set when frame set k's stream carries
   one of them (the caller orders its exchange behind exactly those streams). */
int  swfr_render_resident_group_to(swfr_renderer *r, void *const *block_targets, uint32_t n_frames, uint32_t *sets_used);
void *swfr_stream_handle(swfr_renderer *r, uint32_t set);
int  swfr_wait(swfr_renderer *r);

/* Diagnostics (tools/soak_case.py): copies an intermediate buffer of the last rendered frame to the host.
   what = 0: row headers (8 bytes per (band list entry, row of its tile-row): first cell u32, cells u16, mode u16);
   1: cells (4 bytes each: column relative to the path's x_min << 19 | covered height (5 bits signed) << 14 | uncovered area (14 bits signed));
   2: one uint32, the workgroup size of the k2_bin instance the last launch chain ran (256 or 1024; tests/test_bin_instances_gpu.py).
   Returns the number of bytes copied (at most `bytes`), or a negative SWFR_ERR_*. */
long swfr_debug_copy(swfr_renderer *r, int what, void *dst, size_t bytes);
/* Measurement (tools/cxform_bench.py): the texel pass of colour transforms (cxform.hip) over registered bitmap `bitmap_id` under
   `ct`, `reps` times back to back into a scratch texture, then `reps` device-to-device copies of the same bytes; HIP-event time per
   pass and per copy in *pass_ms / *copy_ms.  Touches no frame and no cache. */
int  swfr_debug_time_cxform(swfr_renderer *r, uint32_t bitmap_id, const swfr_color_transform *ct, uint32_t reps, float *pass_ms, float *copy_ms);
/* Measurement (tools/blur_bench.py): one horizontal and one vertical pass of box width `w` (2..255) over a width x height texture of
   the handle's own, `reps` times each, back to back, then `reps` device-to-device copies of the same bytes; HIP-event time per pass
   and per copy.  Touches no frame and no bitmap. */
int  swfr_debug_time_blur(swfr_renderer *r, uint32_t width, uint32_t height, uint32_t w, uint32_t reps, float *h_ms, float *v_ms, float *copy_ms);
/* Measurement (tools/shadow_bench.py): the two passes of shadow.hip over width x height textures of the handle's own -- the alpha pass
   with offset (dx, dy), the finish pass with a framebuffer-ordered group, in place --, `reps` times each, back to back, then `reps`
   device-to-device copies of the same bytes; HIP-event time per pass and per copy.  Touches no frame and no bitmap. */
int  swfr_debug_time_shadow(swfr_renderer *r, uint32_t width, uint32_t height, int32_t dx, int32_t dy, uint32_t reps, float *alpha_ms, float *finish_ms, float *copy_ms);
/* Measurement (tools/inner_bench.py): swfr_debug_time_shadow with the inner shadow's instances of the two passes -- the inverted alpha
   pass and the inner finish pass (SWFR_SHADOW_INNER alone) --, over the same three textures in the same order. */
int  swfr_debug_time_inner_shadow(swfr_renderer *r, uint32_t width, uint32_t height, int32_t dx, int32_t dy, uint32_t reps, float *alpha_ms, float *finish_ms, float *copy_ms);
/* Measurement (tools/convolve_bench.py): one pass of `kernel` over a width x height texture of the handle's own into another, by the
   framebuffer instance and by the texel instance of convolve.hip, `reps` times each, back to back, then `reps` capture passes
   (k_blur_capture: one read and one write of the same bytes, the streaming roof); HIP-event time per pass.  Touches no frame and no
   bitmap. */
int  swfr_debug_time_convolve(swfr_renderer *r, uint32_t width, uint32_t height, const swfr_kernel *kernel, uint32_t reps, float *fb_ms, float *tex_ms, float *capture_ms);
/* Device pointer of the premultiplied RGBA8 framebuffer (width*height*4 bytes, tight rows). */
void *swfr_device_framebuffer(swfr_renderer *r);

#ifdef __cplusplus
}
#endif
#endif /* SWFR_H */
