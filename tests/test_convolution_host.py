"""Convolution filters on host-only handles (no GPU; DESIGN.md, "Convolution filters"): which kernels swfr_set_kernel takes and which it
refuses, the kernel slots, what a filter entry of kind SWFR_FILTER_CONVOLUTION may carry, the kernel read at the scene walk
(swfr_built_layer_kernel, Renderer.built_filters()), the device primitive's refusals on such a handle, and the Python mirror's own
refusals.
"""
import ctypes as C

import pytest

import convolution_model as cm
import filter_model as fm
import filter_scenes as fsc
import host_frames as hf
import scenarios
from blend_scenes import _rgba
from swf_renderer_amd import api

W, H = 64, 48
BOUND = 8388607
KIDS = [hf.tri((230, 40, 90, 150)), hf.tri((40, 200, 120, 119), dx=9.5)]
DROP = {"color": (10, 20, 60, 200), "dx": 4, "dy": -3, "x": 5, "y": 0, "passes": 3, "strength": 2}
Cv = cm.convolution


def _kernel(width, height, taps):
    k = api.Kernel(width, height)
    for i, t in enumerate(taps):
        k.taps[i] = t
    return k


def _set(r, slot, k):
    return r.L.swfr_set_kernel(r.h, slot, C.byref(k) if k is not None else None), r.L.swfr_last_error(r.h).decode()


def _sid(r):
    return r.register_shape(scenarios._poly_shape([(0, 0), (200, 0), (200, 200)], {"type": "solid", "color": _rgba(9, 9, 9, 100)}))


def _entry(slot, **kw):
    """a Filter array of one convolution entry naming `slot`, with fields changed"""
    arr = (api.Filter * 1)()
    arr[0].kind = api.FILTER_CONVOLUTION
    arr[0].shadow.blur_x = slot
    for k, v in kw.items():
        if k == "color":
            arr[0].shadow.color = api.Rgba8(*v)
        else:
            setattr(arr[0].shadow, k, v)
    return arr


def _set_filters(r, arr, slot=1, count=1):
    return r.L.swfr_set_filters(r.h, slot, arr, count), r.L.swfr_last_error(r.h).decode()


def _walk(r, sid, slot, mode=1):
    return hf.build_raw(r, hf.raw_stage(api.OBJECT_FILTERED_LAYER, mode | slot << 8, sid)[0])[:2]


def _built_kernel(r, k, entry):
    out = api.Kernel()
    rc = r.L.swfr_built_layer_kernel(r.h, k, entry, C.byref(out))
    return rc, (out.width, out.height, list(out.taps[:out.width * out.height]))


def test_the_constants():
    assert api.FILTER_CONVOLUTION == 4 and api.MAX_KERNEL_DIM == 7 and C.sizeof(api.Kernel) == 8 + 49 * 4
    # nothing existing changed its size
    assert C.sizeof(api.Filter) == 4 + C.sizeof(api.Shadow) and C.sizeof(api.Shadow) == 32


def test_accepted_and_refused_kernels():
    r = hf.host(W, H)
    try:
        for w, h in ((1, 1), (7, 7), (1, 7), (7, 1), (2, 2), (4, 6)):
            assert _set(r, 0, _kernel(w, h, [1] * (w * h)))[0] == api.OK, (w, h)
        for w, h in ((0, 1), (1, 0), (0, 0), (8, 1), (1, 8), (8, 8), (2 ** 32 - 1, 1), (1, 2 ** 32 - 1)):
            assert _set(r, 0, _kernel(w, h, [1] * 49)) == (api.ERR_INVALID, "InvalidKernel"), (w, h)
        # the sum of the absolute values at the bound and one past, however it is spread and signed
        for taps, dims in (([BOUND], (1, 1)), ([-BOUND], (1, 1)), ([BOUND - 48] + [1] * 48, (7, 7)), ([-(BOUND - 48)] + [-1] * 24 + [1] * 24, (7, 7)),
                           ([0] * 49, (7, 7)), ([65536], (1, 1))):
            assert _set(r, 0, _kernel(dims[0], dims[1], taps))[0] == api.OK, taps[:2]
        for taps, dims in (([BOUND + 1], (1, 1)), ([-BOUND - 1], (1, 1)), ([BOUND - 47] + [1] * 48, (7, 7)), ([-(BOUND - 47)] + [-1] * 24 + [1] * 24, (7, 7)),
                           ([2 ** 31 - 1], (1, 1)), ([-2 ** 31], (1, 1)), ([-2 ** 31] * 49, (7, 7)), ([2 ** 31 - 1, -2 ** 31], (2, 1))):
            assert _set(r, 0, _kernel(dims[0], dims[1], taps)) == (api.ERR_INVALID, "InvalidKernel"), taps[:2]
        # taps behind width * height are not the kernel's
        assert _set(r, 0, _kernel(1, 1, [65536] + [2 ** 31 - 1] * 48))[0] == api.OK
        # the slot
        assert _set(r, 65535, _kernel(1, 1, [1]))[0] == api.OK
        assert _set(r, 65536, _kernel(1, 1, [1]))[0] == api.ERR_INVALID
        assert _set(r, 7, None)[0] == api.OK                          # clearing an unset slot
        assert r.L.swfr_set_kernel(None, 0, None) == api.ERR_INVALID
    finally:
        r.close()


def test_slots_set_clear_and_a_refused_call_leaves_the_slot():
    r = hf.host(W, H)
    try:
        sid = _sid(r)
        assert _set_filters(r, _entry(5))[0] == api.OK               # (swfr_set_filters does not look at the kernel slot)
        assert _walk(r, sid, 1) == (api.ERR_NOT_FOUND, "KernelNotFound")
        r.set_kernel(5, cm.SHARPEN)
        assert _walk(r, sid, 1)[0] == api.OK
        assert _built_kernel(r, 0, 0) == (api.OK, (3, 3, [t for row in cm.taps_of(cm.SHARPEN) for t in row]))
        # a refused call leaves the slot as it was
        assert _set(r, 5, _kernel(8, 1, [1] * 8)) == (api.ERR_INVALID, "InvalidKernel")
        assert _set(r, 5, _kernel(1, 1, [BOUND + 1])) == (api.ERR_INVALID, "InvalidKernel")
        assert _walk(r, sid, 1)[0] == api.OK and r.built_filters() == [cm.as_dicts([Cv(cm.SHARPEN)])]
        # cleared: the walk refuses by name again, and the slots next to it never held anything
        r.set_kernel(5, None)
        assert _walk(r, sid, 1) == (api.ERR_NOT_FOUND, "KernelNotFound")
        for slot in (4, 6):
            assert _set_filters(r, _entry(slot))[0] == api.OK
            assert _walk(r, sid, 1) == (api.ERR_NOT_FOUND, "KernelNotFound")
    finally:
        r.close()


def test_a_convolution_entry_carries_its_slot_and_nothing_else():
    r = hf.host(W, H)
    try:
        for slot in (65535, 0):                                      # (filter-list slot 1 ends up naming kernel slot 0)
            assert _set_filters(r, _entry(slot))[0] == api.OK, slot
        bad = [dict(blur_x=65536), dict(blur_x=2 ** 32 - 1), dict(blur_y=1), dict(passes=1), dict(dx=1), dict(dy=-1), dict(color=(0, 0, 0, 1)), dict(color=(1, 0, 0, 0)),
               dict(color=(0, 1, 0, 0)), dict(color=(0, 0, 1, 0)), dict(strength=1), dict(flags=1), dict(flags=8)]
        r.set_kernel(0, cm.EDGE)
        sid = _sid(r)
        for kw in bad:
            slot = kw.pop("blur_x", 0)
            assert _set_filters(r, _entry(slot, **kw)) == (api.ERR_INVALID, "InvalidFilter"), kw
            # ... in any place of a list, and the slot keeps what it held
            arr = (api.Filter * 2)(_entry(0)[0], _entry(slot, **kw)[0])
            assert _set_filters(r, arr, 1, 2) == (api.ERR_INVALID, "InvalidFilter"), kw
        assert _walk(r, sid, 1)[0] == api.OK and r.built_filters() == [cm.as_dicts([Cv(cm.EDGE)])]
        # kinds 2 and 3 (and the far ends) are still no kinds, whatever they carry
        for kind in (2, 3, 5, 255, 2 ** 32 - 1):
            arr = _entry(0)
            arr[0].kind = kind
            assert _set_filters(r, arr) == (api.ERR_INVALID, "InvalidFilter"), kind
            arr = api._filter_structs(api.filter_values([fm.blur(5, 4, 2)]))
            arr[0].kind = kind
            assert _set_filters(r, arr) == (api.ERR_INVALID, "InvalidFilter"), kind
        # five entries are still too many
        five = (api.Filter * 5)(*[_entry(0)[0]] * 5)
        assert _set_filters(r, five, 1, 4)[0] == api.OK
        assert _set_filters(r, five, 1, 5) == (api.ERR_CAPACITY, "FilterListLength")
    finally:
        r.close()


def test_the_kernel_is_read_at_the_walk():
    """a slot set anew changes the next walk only; swfr_built_layer_kernel and built_filters() report what the walk read"""
    r = hf.host(W, H)
    try:
        sid = _sid(r)
        r.set_kernel(0, cm.SHARPEN)
        r.set_kernel(9, cm.EVEN_4X6)
        r.set_filters(2, [fm.blur(3, 2, 1), {"convolution": {"slot": 0}}, fm.shadow(DROP), {"convolution": {"slot": 9}}])
        assert _walk(r, sid, 2)[0] == api.OK
        want = cm.as_dicts([fm.blur(3, 2, 1), Cv(cm.SHARPEN), fm.shadow(DROP), Cv(cm.EVEN_4X6)])
        assert r.built_filters() == [want]
        r.set_kernel(0, cm.EMBOSS)                                    # ... the built frame keeps the kernel its walk read
        assert r.built_filters() == [want]
        assert _built_kernel(r, 0, 1) == (api.OK, (3, 3, [t for row in cm.taps_of(cm.SHARPEN) for t in row]))
        assert _built_kernel(r, 0, 3) == (api.OK, (4, 6, [t for row in cm.taps_of(cm.EVEN_4X6) for t in row]))
        # no convolution there, or nothing there at all
        for k, entry in ((0, 0), (0, 2), (0, 4), (1, 0), (2 ** 32 - 1, 1), (0, 2 ** 32 - 1)):
            assert r.L.swfr_built_layer_kernel(r.h, k, entry, None) == api.ERR_NOT_FOUND, (k, entry)
        assert r.L.swfr_built_layer_kernel(r.h, 0, 1, None) == api.OK
        # swfr_built_layer_filters reports the entry as it was set: its kind and its slot
        n, arr = C.c_uint32(), (api.Filter * api.MAX_FILTERS)()
        assert r.L.swfr_built_layer_filters(r.h, 0, C.byref(n), arr) == api.OK and n.value == 4
        assert [(f.kind, f.shadow.blur_x, f.shadow.blur_y, f.shadow.passes) for f in arr[:4]][1::2] == [(4, 0, 0, 0), (4, 9, 0, 0)]
        # the next walk reads the slot anew
        assert _walk(r, sid, 2)[0] == api.OK
        assert r.built_filters() == [cm.as_dicts([fm.blur(3, 2, 1), Cv(cm.EMBOSS), fm.shadow(DROP), Cv(cm.EVEN_4X6)])]
    finally:
        r.close()


def test_built_layer_box_of_a_list_that_starts_with_a_convolution():
    r = hf.host(W, H)
    try:
        r.build_frame({"children": [fsc._filtered(KIDS, [Cv(cm.GAUSS5), fm.blur(5, 4, 2)])]})
        layers = r.built_layers()
        assert len(layers) == 1 and len(layers[0]) == 4 and layers[0][3] == (0, 0, 1)
        assert r.built_filters() == [cm.as_dicts([Cv(cm.GAUSS5), fm.blur(5, 4, 2)])]
        r.build_frame({"children": [fsc._filtered(KIDS, [fm.blur(5, 4, 2), Cv(cm.GAUSS5)])]})
        assert r.built_layers()[0][3] == (5, 4, 2)
        # the sub-frame and the parent's path are a blurred layer's: the kernel changes neither
        a = r.build_frame({"children": [fsc._filtered(KIDS, [Cv(cm.EDGE)], "multiply")]})
        la = r.built_layers()[0]
        b = r.build_frame({"children": [fsc._filtered(KIDS, [fm.blur(3, 3, 1)], "multiply")]})
        lb = r.built_layers()[0]
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and la[0].tobytes() == lb[0].tobytes() and la[1].tobytes() == lb[1].tobytes()
    finally:
        r.close()


def test_the_mirror_allocates_kernel_slots_per_call():
    r = hf.host(W, H)
    try:
        a, b = [Cv(cm.SHARPEN), Cv(cm.EDGE)], [Cv(cm.EDGE), fm.shadow(DROP), Cv(cm.SHARPEN)]
        r.build_frame({"children": [fsc._filtered(KIDS, a), fsc._filtered(KIDS[:1], b), fsc._filtered(KIDS[1:], a, "screen")]})
        assert r.built_filters() == [cm.as_dicts(a), cm.as_dicts(b), cm.as_dicts(a)]
        # two distinct kernels: slots 0 and 1, by first appearance; "matrix" with a divisor and its "taps" are one kernel
        n, arr = C.c_uint32(), (api.Filter * api.MAX_FILTERS)()
        assert r.L.swfr_built_layer_filters(r.h, 1, C.byref(n), arr) == api.OK
        assert [(f.kind, f.shadow.blur_x) for f in arr[:n.value]][::2] == [(4, 1), (4, 0)]
        r.build_frame({"children": [fsc._filtered(KIDS, [Cv(cm.BOX3), Cv(cm.as_dict(cm.BOX3))])]})
        assert r.L.swfr_built_layer_filters(r.h, 0, C.byref(n), arr) == api.OK
        assert [(f.kind, f.shadow.blur_x) for f in arr[:n.value]] == [(4, 0), (4, 0)]
        # a frame without a convolution builds what it built: the other kinds report nothing new
        r.build_frame({"children": [fsc._filtered(KIDS, fsc.CHAIN_OF_FOUR)]})
        assert r.built_filters() == [fm.as_dicts(fsc.CHAIN_OF_FOUR)]
    finally:
        r.close()


def test_the_mirrors_own_refusals():
    r = hf.host(W, H)
    try:
        bad = [{"taps": [[1, 2], [3]]}, {"matrix": [[1, 2], [3]]}, {"taps": [[1]], "matrix": [[1]]}, {}, {"divisor": 2}, {"matrix": [[1]], "divisor": 0},
               {"matrix": [[1]], "divisor": 0.0}, [[1]], None, 5, "sharpen", {"taps": [[1]], "bias": 0}, {"taps": []}, {"taps": [[]]}, {"taps": [1, 2]},
               {"taps": [[1.5]]}, {"taps": [[True]]}, {"matrix": [["1"]]}, {"taps": [[1]], "divisor": 2}, {"taps": [[1] * 8]}, {"taps": [[1]] * 8},
               {"taps": [[2 ** 31]]}, {"matrix": [[1e30]]}, {"matrix": [[float("nan")]]}]
        for value in bad:
            with pytest.raises(api.SwfrError) as e:
                r.build_frame({"children": [fsc._filtered(KIDS, [{"convolution": value}])]})
            assert e.value.code == api.ERR_INVALID and "InvalidFilter" in str(e.value), value
            if value is None:                                         # (set_kernel's way of clearing a slot)
                continue
            with pytest.raises(api.SwfrError) as e:
                r.set_kernel(0, value)
            assert e.value.code == api.ERR_INVALID, value
        # what fits the struct goes to the library, to be refused by name
        for value in ({"taps": [[cm.MAX_ABS_SUM + 1]]}, {"matrix": [[128]]}, {"matrix": [[64, -64]]}):
            with pytest.raises(api.SwfrError) as e:
                r.set_kernel(0, value)
            assert e.value.code == api.ERR_INVALID and "InvalidKernel" in str(e.value), value
            with pytest.raises(api.SwfrError) as e:
                r.build_frame({"children": [fsc._filtered(KIDS, [{"convolution": value}])]})
            assert e.value.code == api.ERR_INVALID and "InvalidKernel" in str(e.value), value
        r.set_kernel(0, {"matrix": [[127.99]]})
        # the rounding of "matrix": floor(m * 65536 / divisor + 0.5)
        assert api.kernel_values({"matrix": [[1, -1, 0.5]], "divisor": 3}) == (3, 1, 21845, -21845, 10923)
        assert api.kernel_values({"matrix": [[1], [2]]}) == (1, 2, 65536, 131072)
        assert api.kernel_values(cm.EVEN_4X6)[2:] == tuple(t for row in cm.taps_of(cm.EVEN_4X6) for t in row)
        # set_filters names kernel slots; a "convolution" value has no place there, nor a slot in a stage
        r.set_filters(0, [{"convolution": {"slot": 65535}}])
        for entry in ({"convolution": cm.SHARPEN}, {"convolution": {"slot": -1}}, {"convolution": {"slot": True}}, {"convolution": {"slot": 1, "taps": [[1]]}}):
            with pytest.raises(api.SwfrError) as e:
                r.set_filters(0, [entry])
            assert e.value.code == api.ERR_INVALID and "InvalidFilter" in str(e.value), entry
        with pytest.raises(api.SwfrError) as e:
            r.set_filters(0, [{"convolution": {"slot": 65536}}])
        assert e.value.code == api.ERR_INVALID and "InvalidFilter" in str(e.value)
        with pytest.raises(api.SwfrError) as e:
            r.build_frame({"children": [fsc._filtered(KIDS, [{"convolution": {"slot": 0}}])]})
        assert e.value.code == api.ERR_INVALID and "InvalidFilter" in str(e.value)
    finally:
        r.close()


def test_the_limits_and_refusals_of_filtered_layers_hold():
    r = hf.host(W, H)
    try:
        one = lambda kids=KIDS: fsc._filtered(kids, [Cv(cm.SHARPEN)])
        r.build_frame({"children": [one() for _ in range(api.MAX_BLUR_LAYERS)]})
        with pytest.raises(api.SwfrError) as e:
            r.build_frame({"children": [one() for _ in range(api.MAX_BLUR_LAYERS + 1)]})
        assert e.value.code == api.ERR_CAPACITY and "BlurLayers" in str(e.value)
        with pytest.raises(api.SwfrError) as e:
            r.build_frame({"children": [one([one()])]})
        assert e.value.code == api.ERR_NOT_IMPLEMENTED and "NestedBlur" in str(e.value)
        with pytest.raises(api.SwfrError) as e:
            r.build_frame({"children": [fsc._filtered(KIDS, [Cv(cm.SHARPEN)] * 5)]})
        assert e.value.code == api.ERR_CAPACITY and "FilterListLength" in str(e.value)
    finally:
        r.close()


def test_convolve_bitmap_on_a_host_only_handle():
    r = hf.host(W, H)
    try:
        k = _kernel(1, 1, [65536])
        assert r.L.swfr_convolve_bitmap(r.h, 3, C.byref(k)) == api.ERR_NO_DEVICE
        # a bad kernel is reported before the missing device
        for bad in (_kernel(0, 1, [1]), _kernel(1, 1, [BOUND + 1])):
            assert r.L.swfr_convolve_bitmap(r.h, 3, C.byref(bad)) == api.ERR_INVALID and r.L.swfr_last_error(r.h).decode() == "InvalidKernel"
        assert r.L.swfr_convolve_bitmap(r.h, 3, None) == api.ERR_INVALID and r.L.swfr_last_error(r.h).decode() == "InvalidKernel"
        with pytest.raises(api.SwfrError) as e:
            r.convolve_bitmap(3, cm.SHARPEN)
        assert e.value.code == api.ERR_NO_DEVICE
    finally:
        r.close()
