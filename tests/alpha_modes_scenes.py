"""Erase and alpha scenes ("Erase and alpha modes"), built from tests/blend_scenes.py, layer_scenes.py, mask_scenes.py and
fade_scenes.py pieces, and their libcairo reference: FadeReplay with CAIRO_OPERATOR_DEST_OUT for the mode "erase" -- as a
"blend_mode" (per path) and as the mode of "layer", "mask" + "layer" and "opacity" + "layer" -- and CAIRO_OPERATOR_DEST_IN for the mode
"alpha", as the mode of those three only.

tools/make_alpha_mode_goldens.py writes goldens() to tests/golden/cairo_alphamode_*.npz (premultiplied RGBA; key = scene name); the
tests rebuild the scenes from here, so a golden file holds pixels only.  Every scene is at most 256 x 64.
"""
import contextlib
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)
import alpha_modes_model as am  # noqa: E402
import blend_model as bm  # noqa: E402
import blend_scenes as bs  # noqa: E402
import fade_scenes as fs  # noqa: E402
import layer_scenes as ls  # noqa: E402
import scenarios  # noqa: E402
from blend_scenes import _rect, _shape  # noqa: E402
from fade_scenes import _faded  # noqa: E402
from layer_scenes import _layer, _pair  # noqa: E402
from mask_scenes import TRANSLUCENT_MASK, _masked, _scaled, _scene  # noqa: E402

MODES = ("erase", "alpha")
LINEAR_BOUND = ls.LINEAR_BOUND               # (no scene here has a linear gradient: every one is exact)
golden_path = bs.golden_path
W, H = 64, 48
# triangles whose pixels tell a SOURCE lerp's 0x7f rounding from OVER's 0x80 (tests/layer_scenes.py, structure_scenes)
FOLLOW = [_shape([(14.6, 7.3), (2.2, 44.1), (41.6, 29.3)], (84, 23, 95, 196)), _shape([(60.4, 43.4), (41.1, 33.1), (9.9, 2.8)], (31, 64, 179, 128))]
CLEAR_FILL = _shape([(2, 2), (60, 5), (30, 44)], (255, 255, 255, 0))


@contextlib.contextmanager
def cairo_operators():
    """the replays of the scenes modules look a mode's cairo_operator_t up in blend_model.CAIRO_OPERATORS: the two modes are in it while
    a scene of this module is drawn"""
    bm.CAIRO_OPERATORS.update(am.CAIRO_OPERATORS)
    try:
        yield
    finally:
        for k in am.CAIRO_OPERATORS:
            del bm.CAIRO_OPERATORS[k]


def cairo_render(sc, aliased=False):
    """premultiplied RGBA of a scene through libcairo"""
    with cairo_operators():
        return fs.cairo_render(sc, aliased)


# ---- scenes
def layer_scenes():
    """erase and alpha layers -- plain, faded, masked -- of overlapping translucent children over an opaque and a translucent ground"""
    out = {}
    for mode in MODES:
        for gname in ("opaque", "translucent"):
            ground = bs._grounds(W, H)[gname]
            out["layer_%s_%s" % (mode, gname)] = _scene(ground + [_layer(mode, _pair())])
            out["faded_%s_%s" % (mode, gname)] = _scene(ground + [_faded(mode, 128, _pair())])
            out["masked_%s_%s" % (mode, gname)] = _scene(ground + [_masked(mode, _pair(), TRANSLUCENT_MASK)])
    return out


def transparent_source_scenes():
    """a layer whose source is transparent everywhere: empty, at opacity 0, masked by an empty mask.  Under alpha the ground goes, under
    erase it stays; the triangles behind show what became of the surface's "still clear" state"""
    out = {}
    tr = bs._grounds(W, H)["translucent"]
    for mode in MODES:
        for gname, ground in (("ground", tr), ("clear", [])):
            out["empty_%s_%s" % (mode, gname)] = _scene(ground + [_layer(mode, [])] + FOLLOW)
            out["opacity0_%s_%s" % (mode, gname)] = _scene(ground + [_faded(mode, 0, _pair())] + FOLLOW)
            out["emptymask_%s_%s" % (mode, gname)] = _scene(ground + [_masked(mode, _pair(), [])] + FOLLOW)
            out["emptycontent_%s_%s" % (mode, gname)] = _scene(ground + [_masked(mode, [], TRANSLUCENT_MASK)] + FOLLOW)
            out["clearfill_%s_%s" % (mode, gname)] = _scene(ground + [_layer(mode, [CLEAR_FILL])] + FOLLOW)
    return out


def erase_path_scenes():
    """ERASE per path: solid colours (opaque, alpha 119, alpha 1; a slanted triangle, an aligned and an unaligned rectangle), bitmap and
    radial sources, a stroke over its own fill, a transparent source"""
    out = {}
    for gname in ("opaque", "translucent"):
        kids = []
        for k, a in enumerate((255, 119, 1)):
            x = 4 + 31 * k
            col = (230 - 60 * k, 40 + 70 * k, 90 + 50 * k, a)
            kids += [_shape([(x + 1.3, 1.2), (x + 27.6, 9.7), (x + 8.2, 30.4)], col), _rect(x + 2, 34, x + 22, 50, col),
                     _rect(x + 3.37, 52.21, x + 24.62, 61.45, col)]
        out["solid_%s" % gname] = _scene(bs._grounds(96, 64)[gname] + [{"type": "container", "blend_mode": "erase", "children": kids}], 96, 64)
    ground = bs._with_ground(dict(width=128, height=64))
    for name, s in (("gradient_radial", 0.5), ("gradient_focal", 0.5), ("bitmap_minified_rotated", 0.6), ("bitmap_repeat_over_solid", 0.5), ("stroke_curves", 0.5)):
        content, bitmaps = _scaled(name, s, 20, 1)
        kw = dict(bitmaps=bitmaps) if bitmaps else {}
        out[name] = _scene(ground + [dict(content, blend_mode="erase")], 128, 64, True, **kw)
    # per path inside a layer (against the layer's own pixels), and an inner "normal" that restores OVER
    out["inside_layer"] = _scene(bs._grounds(W, H)["opaque"] + [_layer("multiply", _pair() + [dict(_rect(10, 10, 40, 40, (0, 0, 0, 128)), blend_mode="erase")])])
    out["normal_inside"] = _scene(bs._grounds(W, H)["opaque"] + [{"type": "container", "blend_mode": "erase", "children": [
        _pair()[0], dict(_pair()[1], blend_mode="normal"), _pair()[2]]}])
    return out


def structure_scenes():
    """what the walk, the rectangle rule and the clear-surface bookkeeping have to get right"""
    out = {}
    ground = bs._grounds(W, H)["opaque"]
    tr = bs._grounds(W, H)["translucent"]
    # ALPHA inside a layer: it clears the layer's surface outside itself, not the frame
    out["alpha_in_layer"] = _scene(ground + [_layer("normal", [_rect(2, 2, 62, 46, (200, 20, 20, 200)), _layer("alpha", _pair())])])
    out["erase_in_layer"] = _scene(ground + [_layer("screen", [_rect(2, 2, 62, 46, (200, 20, 20, 200)), _layer("erase", _pair())])])
    # four levels: the alpha group innermost, and outermost
    for where in ("inner", "outer"):
        kids = _pair(4, 3)
        modes = ("alpha", "multiply", "erase", "normal") if where == "inner" else ("screen", "erase", "add", "alpha")
        for lvl, mode in enumerate(modes):
            kids = [_shape([(3 + 5 * lvl, 3), (50, 8 + 4 * lvl), (10, 40 - 3 * lvl)], (20 + 60 * lvl, 90, 250 - 50 * lvl, 140)), _layer(mode, kids),
                    _rect(40 - 6 * lvl, 30, 62, 46 - 2 * lvl, (250, 250 - 70 * lvl, 20, 120))]
        out["nested4_%s" % where] = _scene(ground + kids)
    # earlier siblings whose rectangles the alpha group's has to take in: small shapes in far corners of a wide frame
    corners = [_shape([(2, 2), (9, 3), (4, 9)], (250, 20, 40, 180)), _shape([(246, 52), (255, 55), (249, 63)], (20, 40, 250, 180))]
    spot = [_shape([(120, 30), (131, 31), (124, 37)], (240, 240, 20, 120)), _rect(100, 20, 150, 50, (9, 90, 200, 100))]
    out["siblings_alpha"] = _scene(corners + [_layer("alpha", spot)], 256, 64)
    out["siblings_alpha_in_layer"] = _scene(corners[:1] + [_layer("normal", corners[1:] + [_layer("alpha", spot)])], 256, 64)
    out["siblings_erase"] = _scene(corners + [_layer("erase", spot)], 256, 64)
    out["siblings_alpha_masked"] = _scene(corners + [_masked("alpha", spot, [_rect(110, 10, 140, 60, (0, 0, 0, 200))])], 256, 64)
    out["siblings_alpha_faded"] = _scene(corners + [_faded("alpha", 77, spot)], 256, 64)
    out["two_alphas"] = _scene(corners + [_layer("alpha", spot + corners[:1]), _shape([(200, 5), (250, 9), (220, 40)], (1, 200, 2, 200)), _layer("alpha", _pair(150, 10))], 256, 64)
    # alpha groups inside a masked layer's halves
    out["alpha_in_content"] = _scene(ground + [_masked("normal", [_rect(2, 2, 62, 46, (200, 20, 20, 200)), _layer("alpha", _pair())], TRANSLUCENT_MASK)])
    out["alpha_in_mask"] = _scene(ground + [_masked("normal", _pair(), [_rect(2, 2, 62, 46, (0, 0, 0, 255)), _layer("alpha", TRANSLUCENT_MASK)])])
    # opaque covers: inside an erase group they hide nothing; an erase path above and below an opaque full cover
    out["cover_inside"] = _scene([_rect(0, 0, 128, 48, (30, 160, 90, 255)), _layer("erase", [_rect(0, 0, 128, 48, (60, 50, 20, 255)), _shape([(5, 3), (120, 10), (90, 45)], (250, 200, 40, 200))]),
                                  _shape([(50, 2), (126, 20), (60, 46)], (255, 255, 255, 90))], 128, 48)
    out["cover_between"] = _scene([dict(_shape([(5, 3), (120, 10), (90, 45)], (250, 200, 40, 200)), blend_mode="erase"), _rect(0, 0, 128, 48, (30, 160, 90, 255)),
                                   dict(_shape([(50, 2), (126, 20), (60, 46)], (255, 255, 255, 90)), blend_mode="erase")], 128, 48)
    out["alpha_over_cover"] = _scene([_rect(0, 0, 128, 48, (30, 160, 90, 255)), _layer("alpha", _pair(20, 2))], 128, 48)
    # a group partly off the frame
    out["offframe_part"] = _scene(tr + [_layer("erase", _pair(30, 20)), _layer("alpha", _pair(-25, -22))])
    # ---- the clear-surface bookkeeping: an erase or alpha operation on a still-clear surface changes no pixel, and the translucent
    #      triangles behind it are composited with OVER all the same (probed: the five preludes, and an erase with a transparent source)
    out["first_erase_path"] = _scene([dict(_pair()[0], blend_mode="erase")] + FOLLOW)
    out["first_erase_layer"] = _scene([_layer("erase", _pair())] + FOLLOW)
    out["first_alpha_layer"] = _scene([_layer("alpha", _pair())] + FOLLOW)
    out["first_alpha_empty"] = _scene([_layer("alpha", [])] + FOLLOW)
    out["paint_erase_all"] = _scene([_rect(0, 0, 64, 48, (9, 99, 199, 255)), dict(_rect(0, 0, 64, 48, (0, 0, 0, 255)), blend_mode="erase")] + FOLLOW)
    out["first_erase_clear_source"] = _scene([dict(CLEAR_FILL, blend_mode="erase")] + FOLLOW)
    out["first_erase_opacity0"] = _scene([_faded("erase", 0, _pair())] + FOLLOW)
    out["first_erase_emptymask"] = _scene([_masked("erase", _pair(), [])] + FOLLOW)
    return out


PRELUDES = ("first_erase_path", "first_erase_layer", "first_alpha_layer", "first_alpha_empty", "paint_erase_all", "first_erase_clear_source")


def files():
    """golden file name -> (scenes, aliased)"""
    out = {}
    for aliased in (False, True):
        a = "aliased_" if aliased else ""
        out["cairo_alphamode_%slayers" % a] = (layer_scenes, aliased)
        out["cairo_alphamode_%stransparent" % a] = (transparent_source_scenes, aliased)
        out["cairo_alphamode_%spaths" % a] = (erase_path_scenes, aliased)
        out["cairo_alphamode_%sstructure" % a] = (structure_scenes, aliased)
    return out


def goldens():
    return {fname: {name: cairo_render(sc, aliased) for name, sc in sorted(make().items())} for fname, (make, aliased) in files().items()}


# ---- random trees
def rand_alpha_mode_scene(rng, **kw):
    """fade_scenes.rand_faded_scene -- random composited trees with layers, blend modes, colour transforms, masks and opacities -- with
    the two modes put at random where a handle with SWFR_FLAG_ALPHA_MODES takes them: "erase" as a "blend_mode" and as the mode of any
    layer, "alpha" as the mode of a layer (an object that has "layer", "mask" or "opacity")"""
    sc = fs.rand_faded_scene(rng, **kw)

    def visit(obj):
        if obj.get("blend_mode") is not None and rng.integers(0, 3) == 0:
            obj["blend_mode"] = "erase"
        layered = obj.get("layer") not in (None, False) or obj.get("mask") is not None or obj.get("opacity") is not None
        if layered and rng.integers(0, 2) == 0:
            obj["layer"] = MODES[int(rng.integers(0, 2))]
        for c in obj.get("children", []):
            visit(c)
        for c in obj.get("mask") or []:
            visit(c)
    for k in sc["stage"]["children"]:
        visit(k)
    return sc


FUZZ_SEEDS = 6200                                                  # (tests/test_alpha_modes_host.py holds them against a host-only handle)


def fuzz_scene(seed, aliased):
    """the frames of tests/test_alpha_modes_gpu.py's differential fuzz"""
    import numpy as np
    return rand_alpha_mode_scene(np.random.default_rng(FUZZ_SEEDS + seed + 100 * aliased))


def build_flagged(sc, aliased=False):
    """swfr_build_frame's arrays (edges, paths, styles) for the scene from a host-only handle with SWFR_FLAG_ALPHA_MODES"""
    import host_frames as hf
    r = hf.host(sc["width"], sc["height"], even_odd=bool(sc.get("even_odd")), antialias="none" if aliased else "default", alpha_modes=True)
    try:
        for b in sc.get("bitmaps", []):
            r.add_bitmap(b)
        for bid, (w, h, px) in sc.get("raw_bitmaps", {}).items():
            r.register_bitmap(bid, w, h, px)
        return r.build_frame(sc["stage"])
    finally:
        r.close()


def buildable(sc, aliased=False):
    """build_flagged, or None where the host refuses the frame for capacity (the random modes and opacities can nest too deep)"""
    from swf_renderer_amd import api
    try:
        return build_flagged(sc, aliased)
    except api.SwfrError as e:
        if e.code != api.ERR_CAPACITY:
            raise
        return None
