// renderer.cpp -- the C-ABI of include/swfr.h: handle, asset store, host frame build, device pipeline.
//
// There is NO CPU rasterization fallback in this library: without a HIP device swfr_create fails
// (unless the caller explicitly asks for a host-only handle, which can decode and build edge lists
// but refuses to render).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <functional>
#include <initializer_list>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/swfr.h"
#include "device_types.hpp"
#include "frame_layout.hpp"
#include "filter_plan.hpp"
#include "frame_builder.hpp"
#include "shape_decoder.hpp"
#include "bitmap_decode.hpp"

namespace swfr {
void launch2_bin(hipStream_t, const Frame2*, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, bool, uint32_t);
void launch2_rows(hipStream_t, const Frame2*, uint32_t, uint32_t, uint32_t, bool, bool);
bool rows_wide_instance(uint32_t, bool);
void launch2_rows_ahead(hipStream_t, const Frame2*, const Frame2*, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t);
void launch2_rows_slow(hipStream_t, const Frame2*, uint32_t, uint32_t, uint32_t, uint32_t, bool);
void launch2_tiles(hipStream_t, const Frame2*, uint32_t, uint32_t, uint32_t, int, uint32_t*);
void launch2_linear_pieces(hipStream_t, const Frame2*, uint32_t, uint32_t);
void launch_unpremultiply(hipStream_t, const uint32_t*, uint32_t*, size_t);
void launch_pack_band(hipStream_t, const uint32_t*, uint32_t*, int, int, uint32_t, uint32_t, uint32_t);
void launch_cxform_texels(hipStream_t, const uint8_t*, uint32_t*, size_t, const uint32_t*);
void launch_blur_capture(hipStream_t, const uint32_t*, uint32_t*, size_t);
void launch_blur_pass(hipStream_t, const uint32_t*, uint32_t*, uint32_t, uint32_t, uint32_t, bool);
void launch_shadow_alpha(hipStream_t, const uint32_t*, uint32_t*, uint32_t, uint32_t, int32_t, int32_t, bool);
void launch_shadow_finish(hipStream_t, const uint32_t*, const uint32_t*, bool, uint32_t*, size_t, uint32_t, uint32_t, uint32_t);
void launch_convolve(hipStream_t, const uint32_t*, uint32_t*, uint32_t, uint32_t, const swfr_kernel&, bool);   // convolve.hip
}  // namespace swfr

using namespace swfr;

namespace {

constexpr size_t COUNTER_WORDS = C2_WORDS;   // per frame set

struct HipError {
    hipError_t code;
    const char* what;
};
#define HIP_CHECK(expr)                                 \
    do {                                                \
        hipError_t _e = (expr);                         \
        if (_e != hipSuccess) throw HipError{_e, #expr}; \
    } while (0)

// grow-only device buffer
template <class T>
struct DevBuf {
    T* ptr = nullptr;
    size_t cap = 0;
    void reserve(size_t n) {
        if (n <= cap) return;
        if (ptr) HIP_CHECK(hipFree(ptr));
        ptr = nullptr;
        cap = 0;
        size_t want = std::max<size_t>(n, 64);
        want += want / 2;
        HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&ptr), want * sizeof(T)));
        cap = want;
    }
    void release() {
        if (ptr) (void)hipFree(ptr);
        ptr = nullptr;
        cap = 0;
    }
};

// A scene as every host function sees it: the three arrays of the C ABI (swfr_upload_edges) or of the frame builder, or what
// prepare_frame made of them.  A view: it owns nothing.
struct SceneView { const swfr_edge* edges; size_t n_edges; const swfr_path* paths; size_t n_paths; const swfr_style* styles; size_t n_styles; };

// What the kernels of a frame -- or of several frames per launch (blockIdx.y = frame) -- are launched with: the grids' bounds over the
// frames of the launch (plan_bounds, merge_bounds), and the choices in which the routes differ.
struct LaunchPlan {
    uint32_t max_edges, max_paths, max_bands, slow_kernels;      // k2_bin; slow_kernels 1: it also prepares the queued-row kernels' work
    uint32_t bin_threads;                                        // k2_bin's instance: BIN_THREADS_SMALL or BIN_THREADS_LARGE (bin_threads_of)
    uint32_t max_chunks, max_path_edges; bool rows_wide;         // the row pass
    bool run_slow; uint32_t grid_slow, grid_huge, slow_passes;   // the queued-row kernels (coincident edges, crowded rows), if launched
    uint32_t linear_grid;                                        // k2_linear_pieces (0: not launched)
    uint32_t max_strips, tiles_grid; int shader_level;           // the tile pass; tiles_grid ~0u: the default shape, any other value caps the wavefronts
};

// The read-only arrays of an uploaded scene live in one device allocation and are filled by one H2D copy from one pinned
// staging buffer (nine small pageable copies cost ~70 us of host time per frame; one pinned copy a fraction of that).
struct SceneArena {
    uint8_t* dev = nullptr;
    uint8_t* host = nullptr;
    size_t cap = 0, used = 0;
    hipEvent_t copied = nullptr;             // recorded behind the H2D: the staging buffer may be rewritten after it
    hipEvent_t copy_begin = nullptr, copy_end = nullptr;   // timing of the copy (swfr_last_path_timing)
    void begin(size_t bytes) {
        if (copied) HIP_CHECK(hipEventSynchronize(copied));
        if (bytes > cap) {
            if (dev) (void)hipFree(dev);
            if (host) (void)hipHostFree(host);
            dev = host = nullptr;
            const size_t want = bytes + bytes / 2 + 4096;
            HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&dev), want));
            HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&host), want, hipHostMallocDefault));
            cap = want;
        }
        used = 0;
    }
    static size_t padded(size_t bytes) { return (bytes + 255) & ~size_t(255); }
    // copies `bytes` into the staging buffer and returns the device address they will land at
    void* push(const void* src, size_t bytes) {
        void* d = dev + used;
        if (bytes && src) std::memcpy(host + used, src, bytes);     // (src == nullptr: the caller has written the bytes in place)
        used += padded(bytes);
        return d;
    }
    void flush(hipStream_t st, bool timed = false) {
        if (timed) {
            if (!copy_begin) { HIP_CHECK(hipEventCreate(&copy_begin)); HIP_CHECK(hipEventCreate(&copy_end)); }
            HIP_CHECK(hipEventRecord(copy_begin, st));
        }
        if (used) HIP_CHECK(hipMemcpyAsync(dev, host, used, hipMemcpyHostToDevice, st));
        if (timed) HIP_CHECK(hipEventRecord(copy_end, st));
        if (!copied) HIP_CHECK(hipEventCreateWithFlags(&copied, hipEventDisableTiming));
        HIP_CHECK(hipEventRecord(copied, st));
    }
    void release() {
        if (copied) (void)hipEventDestroy(copied);
        if (copy_begin) { (void)hipEventDestroy(copy_begin); (void)hipEventDestroy(copy_end); }
        if (dev) (void)hipFree(dev);
        if (host) (void)hipHostFree(host);
        dev = host = nullptr; copied = nullptr; copy_begin = copy_end = nullptr; cap = used = 0;
    }
};

struct DeviceBitmap {
    uint32_t* pixels = nullptr;
    uint32_t width = 0, height = 0;
    uint64_t gen = 0;                        // registration generation: a colour-transformed texture is made from one generation
    std::vector<uint8_t> straight;           // the straight RGBA8 texels as registered (tight rows), for the texel pass
    uint8_t* d_straight = nullptr;           // ... on the device: uploaded the first time a colour transform uses the bitmap (kept until the
                                             // bitmap is registered again; not counted against SWFR_CXFORM_CACHE_MB)
    hipEvent_t straight_ready = nullptr;     // recorded behind that upload, on straight_stream
    hipStream_t straight_stream = nullptr;
    bool straight_done = false;              // the upload is known to have completed
    bool captured = false;                   // made on the device (swfr_capture_bitmap, swfr_blur_bitmap): premultiplied texels only, no `straight`
};

// A colour-transformed texture (cxform.hip): premultiplied ARGB of one (bitmap, generation, chain), made by the texel pass on `stream`
// (`ready` recorded behind it).  Kept in the handle's cache under a byte budget (SWFR_CXFORM_CACHE_MB); never evicted while the call
// that uses it runs (used_epoch) or while it belongs to the resident scene (pinned).
struct CxVariant {
    uint32_t* pixels = nullptr;
    size_t bytes = 0;
    uint32_t bitmap = 0;
    uint64_t gen = 0;
    hipEvent_t ready = nullptr;
    hipStream_t stream = nullptr;
    bool done = false;                       // `ready` known to have completed
    bool pinned = false;
    uint64_t used_epoch = 0, last_use = 0;
    std::shared_ptr<uint32_t> table;         // the chain's packed table as copied behind the texels (kept: the copy is queued on `stream`)
};

}  // namespace

struct swfr_renderer {
    uint32_t width = 0, height = 0;
    swfr_config cfg{};
    bool has_device = false;
    std::string error;
    std::unique_ptr<FrameBuilder> builder;
    std::string json_scratch;

    // device state
    hipStream_t stream = nullptr;           // == fs[0].stream
    uint32_t* h_counters = nullptr;         // pinned: the kernels' counters of up to four frame sets
    std::vector<hipEvent_t> ev;             // 4 per frame of the last swfr_render_resident call
    // The read-only arrays of one uploaded scene (views into its arena) and what the launches need to know about it.
    // Resident rendering uses scene 0; swfr_render_batch keeps one scene per frame in flight.
    struct Scene {
        SceneArena arena;
        FrameDims dims;                           // what the sizes of a frame's kernel-written buffers follow from (frame_layout.hpp)
        LaunchPlan bounds{};                      // the grids' bounds of a frame of the scene (plan_bounds); plan_of adds what a launch chooses
        Frame2 proto{};                           // the scene fields and sizes of a frame descriptor (per-frame buffers not filled in)
        Frame2* frames_dev = nullptr;            // one descriptor per frame set (contiguous, in the arena): parity 0, what every route launches with
        Frame2* frames_ahead = nullptr;          // ... and the sets' parity-1 descriptors, when the upload made them (upload2): k2_bin's buffers a second time, the rest shared
        uint32_t slow_passes = SLOW_PASSES;      // passes of the slow-row kernels the scene needs (known after a frame of a resident scene)
        bool slow_verified = false;              // slow_state / slow_passes come from this scene's own counters, not from the previous scene
        int slow_state = 0;                      // 0: unknown (both slow-row kernels are launched), 1: the scene has no queued rows, 2: none with > 64 edges
    };
    Scene scn[4];
    // One set of kernel-written per-frame buffers and the stream they are used on.  With SWFR_FRAMES_IN_FLIGHT = n consecutive
    // frames rotate over n sets, so the front of frame f+1 overlaps the tail of frame f (every frame recomputes everything).
    struct FrameSet {
        hipStream_t stream = nullptr;
        DevBuf<uint8_t> work, cls;               // the kernel-written buffers of one frame, carved like a batch group's (place_frame)
        DevBuf<uint32_t> strip_cost;             // ... but the strip costs, which stay where they are from scene to scene (upload2)
        DevBuf<uint32_t> strip_cost_ahead;       // ... and parity 1's
        uint32_t* counters = nullptr;            // this set's COUNTER_WORDS of swfr_renderer::d_counters (one buffer: one copy brings all sets' back)
        DevBuf<uint32_t> d_fb;
        // the kernels of one frame of the resident scene on this set, captured once per uploaded scene: a frame is then ONE
        // hipGraphLaunch for the host instead of three to twelve kernel launches
        hipGraph_t graph = nullptr;
        hipGraphExec_t graph_exec = nullptr;
        uint64_t graph_key = 0;                  // scene generation | slow_state | slow_passes the graph was captured for (0: none)
    };
    FrameSet fs[4];
    uint64_t scene_gen = 0;                 // counts uploads into scene slot 0
    int resident_batch = 2;                 // SWFR_RESIDENT_BATCH: frames per kernel launch of swfr_render_resident (blockIdx.y = frame; 0/1: one launch chain per frame).
                                            // Two since round 4 (calls without per-kernel events only): half the launches fill the pipeline sooner -- 20 frames 640 us instead of 690,
                                            // 300 frames alike (tools/short_run_probe.py); four per launch lose the overlap of consecutive groups (33.9 us per frame)
#ifdef SWFR_EMU
    int use_graphs = 0;                     // (the emulator's runtime has no graphs)
#else
    int use_graphs = 0;                     // SWFR_GRAPHS=1: frames of a resident scene as graph launches.  Off by default: measured on MI355X /
                                            // ROCm 7.2 a graph launch per frame is SLOWER than its three kernel launches (S1: 162 000 instead of
                                            // 218 000 Mpx/s at 300 frames, 143 000 instead of 178 000 at 20: profiles/r03p_graphs.txt)
#endif
    DevBuf<DevBitmap> d_bitmap_table;
    DevBuf<uint32_t> d_tmp;
    DevBuf<uint32_t> d_counters;            // 8 x COUNTER_WORDS: the frame sets' counters, contiguous, and behind them those of the sets' parity-1 descriptors
    int in_flight = 4;
    bool scene_from_builder = false;        // the scene in slot 0 is the frame builder's last frame (its arrays are still there)
    uint32_t sets_ready = 0;                // frame sets whose descriptors belong to the scene in slot 0 (swfr_render prepares one, swfr_upload_edges all)
    int hint_slow_state = 0; uint32_t hint_slow_passes = SLOW_PASSES;   // what the last rendered scene needed of the queued-row kernels
    uint32_t* fb_cur = nullptr;             // framebuffer of the last completed frame
    std::map<uint32_t, DeviceBitmap> bitmaps;
    std::vector<DevBitmap> bitmap_table;   // indexed by bitmap id
    uint64_t bitmap_gen = 0;
    // colour-transformed textures: key = bitmap id | generation | the chain's 1 024 table bytes
    std::unordered_map<std::string, CxVariant> cx_cache;
    size_t cx_bytes = 0, cx_budget = size_t(512) << 20;   // SWFR_CXFORM_CACHE_MB
    uint64_t cx_epoch = 0, cx_tick = 0, cx_synced_epoch = ~uint64_t(0);
    std::vector<std::string> cx_pins;      // the resident scene's textures
    std::vector<DevBitmap> variant_table;  // textures VARIANT_BASE + k of the scene being laid out
    // blurred layers ("Blurred layers"): texture BLUR_BASE + k of the frame swfr_render is drawing -- a grow-only pool, of the
    // frame's size each, valid until the handle's next scene walk -- and the scratch texture the passes alternate with
    DevBuf<uint32_t> blur_tex[SWFR_MAX_BLUR_LAYERS];
    DevBuf<uint32_t> blur_scratch;
    DevBuf<uint32_t> shadow_scratch;       // swfr_shadow_bitmap, and a shadow behind another filter: the alpha surface, which alternates with blur_scratch
    std::vector<DevBitmap> blur_table;
    bool bitmap_table_dirty = false, bitmap_table_dirty_copied = false;
    bool scene_ready = false, fb_valid = false;
    swfr_timing timing{};
    swfr_path_timing path_timing{};
    int force_chunk_rows = 0;               // SWFR_CHUNK_ROWS: test knob
    int strip_order = 1;                    // SWFR_STRIP_ORDER=0: launch the k2_tiles wavefronts in row-major order (per XCD class)
    int event_stride = 16;                  // SWFR_EVENT_STRIDE: per-kernel HIP events on every n-th resident frame
    bool event_stride_given = false;        // (set explicitly: short runs do not lower it)
    bool mono = false;                      // SWFR_FLAG_ANTIALIAS_NONE: boxes rounded to pixels, tor paths by k2_rows_mono (Frame2::mono)
    int fast_limit = 16;                    // rows with more active edges go to k2_rows_slow; the row kernel's instance caps it at its 8 or 16 slots (SWFR_FAST_LIMIT: test knob)
    int tiles_grid = 0;                     // SWFR_TILES_GRID: persistent k2_tiles wavefronts per frame (0 = default)
    int bin_threads = 0;                    // SWFR_BIN_THREADS: 256 or 1024 forces that instance of k2_bin (0 = the launch plan's rule; tests and sweeps)
    uint32_t last_bin_threads = 0;          // the instance of the last launch chain (swfr_debug_copy, what = 2)
    int bin_ahead = 1;                      // SWFR_BIN_AHEAD=0: every frame of swfr_render_resident is bin -> rows -> tiles; 1: where the call allows it, the next frame
                                            // of a frame set is binned in the row launch of the one before (render_resident)
    uint32_t last_ahead_launches = 0;       // k2_rows_ahead_b launches of the last swfr_render_resident call (swfr_debug_copy, what = 3)
    int tiles_shaders = 0;                  // SWFR_TILES_SHADERS: the lowest k2_tiles instance a frame runs (0 solid, 1 bitmap, 2 shaded, 3 blend operators, 4 isolated groups, 5 masked groups, 6 faded groups, 7 erase and alpha operators; test knob)
    bool rows_wide = false;                 // SWFR_ROWS_WIDE=1: every frame with tor paths runs k2_rows_wide (test knob; aliased frames keep k2_rows_mono)
    // swfr_render_batch: groups of frames rendered by ONE launch per kernel (blockIdx.y = frame); two groups alternate,
    // the host builds one while the GPU works on the other
    struct BatchGroup {
        SceneArena arena;                   // the frames' edge lists, tables and descriptors: one H2D copy per group
        DevBuf<uint8_t> work, cls;          // the kernel-written buffers of every frame of the group, carved from two allocations
        hipStream_t stream = nullptr;
        uint32_t* h_counters = nullptr;     // pinned
        size_t h_counters_cap = 0;
        hipEvent_t ev_begin = nullptr, ev_end = nullptr;   // around the group's kernels
    };
    BatchGroup groups[2];
    int batch_frames = 64;                  // SWFR_BATCH_FRAMES: frames per launch in swfr_render_batch
    uint32_t* targets[4] = {nullptr, nullptr, nullptr, nullptr};   // swfr_set_targets: frame set k renders into targets[k]
    swfr_stats stats = {};
    // swfr_render_resident_batched: B copies of the kernel-written buffers + B framebuffers, the B descriptors, events
    DevBuf<uint8_t> rb_work, rb_cls;
    DevBuf<Frame2> rb_frames;
    DevBuf<uint32_t> rb_fb;
    hipEvent_t rb_ev[2] = {nullptr, nullptr};
    // swfr_read_image: pinned staging (a pageable destination costs 7x the copy time), swfr_read_image_async: the copy in flight
    uint8_t* h_image = nullptr; size_t h_image_cap = 0;
    hipEvent_t read_done = nullptr;
    bool read_pending = false;
    uint32_t n_targets = 0, async_next = 0, async_used = 0;   // async_used: bit k = frame set k has run since the last wait

    ~swfr_renderer() {
        if (has_device) {
            (void)hipSetDevice(cfg.device);
            d_bitmap_table.release(); d_tmp.release(); d_counters.release();
            rb_work.release(); rb_cls.release(); rb_frames.release(); rb_fb.release();
            for (auto& t : blur_tex) t.release();
            blur_scratch.release(); shadow_scratch.release();
            for (auto& e : rb_ev) if (e) (void)hipEventDestroy(e);
            if (h_image) (void)hipHostFree(h_image);
            if (read_done) (void)hipEventDestroy(read_done);
            for (int k = 0; k < 4; ++k) {
                FrameSet& x = fs[k];
                x.work.release(); x.cls.release(); x.strip_cost.release(); x.strip_cost_ahead.release(); x.d_fb.release();
                if (x.graph_exec) (void)hipGraphExecDestroy(x.graph_exec);
                if (x.graph) (void)hipGraphDestroy(x.graph);
                if (k > 0 && x.stream) (void)hipStreamDestroy(x.stream);
                scn[k].arena.release();
            }
            if (h_counters) (void)hipHostFree(h_counters);
            for (auto& g : groups) {
                g.arena.release(); g.work.release(); g.cls.release();
                if (g.stream) (void)hipStreamDestroy(g.stream);
                if (g.h_counters) (void)hipHostFree(g.h_counters);
                if (g.ev_begin) { (void)hipEventDestroy(g.ev_begin); (void)hipEventDestroy(g.ev_end); }
            }
            for (auto& kv : bitmaps) {
                if (kv.second.pixels) (void)hipFree(kv.second.pixels);
                if (kv.second.d_straight) (void)hipFree(kv.second.d_straight);
                if (kv.second.straight_ready) (void)hipEventDestroy(kv.second.straight_ready);
            }
            for (auto& kv : cx_cache) {
                if (kv.second.pixels) (void)hipFree(kv.second.pixels);
                if (kv.second.ready) (void)hipEventDestroy(kv.second.ready);
            }
            for (auto& e : ev) if (e) (void)hipEventDestroy(e);
            if (stream) (void)hipStreamDestroy(stream);
        }
    }
};

namespace {

int fail(swfr_renderer* r, int code, const std::string& msg) {
    if (r) r->error = msg;
    return code;
}

template <class F>
int guarded(swfr_renderer* r, F&& f) {
    try {
        if (r && r->has_device) HIP_CHECK(hipSetDevice(r->cfg.device));
        return f();
    } catch (const StatusError& e) {
        return fail(r, e.code, e.message);
    } catch (const HipError& e) {
        return fail(r, SWFR_ERR_DEVICE, std::string(e.what) + ": " + hipGetErrorString(e.code));
    } catch (const std::bad_alloc&) {
        return fail(r, SWFR_ERR_CAPACITY, "out of host memory");
    } catch (const std::exception& e) {
        return fail(r, SWFR_ERR_INVALID, e.what());
    }
}

// the frame builder's last frame (its edges carry their path index in `reserved`)
SceneView builder_view(const swfr_renderer* r) {
    const auto& e = r->builder->edges(); const auto& p = r->builder->paths(); const auto& s = r->builder->styles();
    return SceneView{e.data(), e.size(), p.data(), p.size(), s.data(), s.size()};
}

// the frame sets a handle rotates its frames over (SWFR_FRAMES_IN_FLIGHT, 1..4): what an upload into every set prepares
uint32_t sets_wanted(const swfr_renderer* r) { return uint32_t(std::max(1, std::min(r->in_flight, 4))); }
// ... and how many of them hold descriptors and buffers of the resident scene: what a call may rotate over now.  (upload2 gives every
// set below sets_ready its stream, its work buffer and -- on a handle without caller targets -- its framebuffer, and swfr_set_targets
// asks for a new upload: the buffer test only ever ends the count where sets_ready does)
uint32_t sets_of_scene(const swfr_renderer* r) {
    uint32_t n = 1;
    while (n < sets_wanted(r) && n < r->sets_ready && r->fs[n].stream && r->fs[n].work.ptr) ++n;
    return n;
}

// the handle's share of the frame's tile-rows: local tile-row l is frame tile-row first + l * stride, l < count; `padded` = the
// share of the best-served rank (slabs are gathered at that common size)
struct BandShare { uint32_t first, stride, count, padded; };
BandShare band_share(const swfr_renderer* r) {
    const uint32_t tile_rows = (r->height + TILE_H - 1) / TILE_H;
    const uint32_t bc = r->cfg.band_count > 1 ? r->cfg.band_count : 1, bi = r->cfg.band_count > 1 ? r->cfg.band_index : 0;
    if (bc > 1 && (r->cfg.flags & SWFR_FLAG_BANDS_CONTIGUOUS)) {
        const uint32_t n = (tile_rows + bc - 1) / bc, first = bi * n;
        return BandShare{first, 1u, first >= tile_rows ? 0u : std::min(n, tile_rows - first), n};
    }
    return BandShare{bi, bc, tile_rows <= bi ? 0u : (tile_rows - bi + bc - 1) / bc, (tile_rows + bc - 1) / bc};
}
uint32_t local_tile_rows(const swfr_renderer* r) { return band_share(r).count; }

// swfr_path::lerp is lerp | operator << 8: an operator is never a SOURCE lerp
// (alpha_modes, SWFR_FLAG_ALPHA_MODES: SWFR_OP_ERASE is an operator like the eight; SWFR_OP_ALPHA, which is unbounded, is a GROUP_END's only)
void validate_blend_fields(const SceneView& sv, bool alpha_modes) {
    for (size_t i = 0; i < sv.n_paths; ++i) {
        const uint32_t v = sv.paths[i].lerp;
        if (sv.paths[i].kind >= SWFR_PATH_GROUP_BEGIN) continue;      // (validate_groups)
        if (alpha_modes && (v >> 8) == SWFR_OP_ALPHA) throw StatusError{SWFR_ERR_INVALID, "path blend field: SWFR_OP_ALPHA is the operator of a GROUP_END only"};
        if (alpha_modes && v == uint32_t(SWFR_OP_ERASE) << 8) continue;
        if ((v & 0xffu) > 1u || (v >> 8) > SWFR_OP_HARDLIGHT || ((v >> 8) != 0u && (v & 0xffu) != 0u))
            throw StatusError{SWFR_ERR_INVALID, "path blend field: lerp must be 0 or 1, the operator at most 8, and lerp 0 with an operator"};
    }
}

// the markers of isolated groups (swfr.h, SWFR_PATH_GROUP_BEGIN / _END / _MASK): balanced, at most SWFR_MAX_LAYER_DEPTH deep -- a group
// with a MASK counting two levels from its BEGIN on --, no edges, the markers' rectangles equal, every path between them inside that
// rectangle, the lerp bits zero, END's operator one of SWFR_OP_*, at most one MASK per group and none outside one.  Bits 24..31 of an
// END's lerp are the group's fade (255 - opacity, swfr.h): on a group without a MASK only, and on no other path (a BEGIN's and a MASK's
// lerp is 0 as a whole; an ordinary path's is refused by validate_blend_fields)
// alpha_modes (SWFR_FLAG_ALPHA_MODES): END's operator may be SWFR_OP_ERASE or SWFR_OP_ALPHA, and the rectangle of an ALPHA group
// contains the rectangle of every path drawn since the surface the group is composited onto began -- its enclosing GROUP_BEGIN (or
// GROUP_MASK: the mask's surface), or the frame's start: the composite clears that surface wherever the group is transparent
void validate_groups(const SceneView& sv, bool alpha_modes) {
    const swfr_path* const paths = sv.paths; const size_t n_paths = sv.n_paths;
    auto bad =[](const char* what) { throw StatusError{SWFR_ERR_INVALID, what}; };
    const uint32_t max_op = alpha_modes ? uint32_t(SWFR_OP_ALPHA) : uint32_t(SWFR_OP_HARDLIGHT);
    PixelRect seen[SWFR_MAX_LAYER_DEPTH + 1];                    // per open surface: the union of the rectangles drawn onto it so far
    // which BEGINs open a masked group (a MASK belongs to the innermost group open where it stands)
    static thread_local std::vector<size_t> opened;
    static thread_local std::vector<uint8_t> masked;
    opened.clear();
    bool any_mask = false;
    for (size_t i = 0; i < n_paths && !any_mask; ++i) any_mask = paths[i].kind == SWFR_PATH_GROUP_MASK;
    if (any_mask) {
        masked.assign(n_paths, 0);
        for (size_t i = 0; i < n_paths; ++i) {
            const uint32_t kind = paths[i].kind;
            if (kind == SWFR_PATH_GROUP_BEGIN) opened.push_back(i);
            else if (kind == SWFR_PATH_GROUP_END) { if (!opened.empty()) opened.pop_back(); }
            else if (kind == SWFR_PATH_GROUP_MASK) {
                if (opened.empty()) bad("GROUP_MASK outside a group");
                if (masked[opened.back()]) bad("a second GROUP_MASK in one group");
                masked[opened.back()] = 1;
            }
        }
    }
    size_t open[SWFR_MAX_LAYER_DEPTH];
    int depth = 0, levels = 0;
    for (size_t i = 0; i < n_paths; ++i) {
        const swfr_path& p = paths[i];
        if (depth) {
            const swfr_path& g = paths[open[depth - 1]];
            if (p.x_min < g.x_min || p.y_min < g.y_min || p.x_max > g.x_max || p.y_max > g.y_max)
                bad(p.kind >= SWFR_PATH_GROUP_END ? "group markers: the rectangles of GROUP_BEGIN and GROUP_END differ" : "a path lies outside the rectangle of its group");
        }
        if (p.kind > SWFR_PATH_GROUP_MASK) bad("unknown path kind");
        if (p.kind == SWFR_PATH_GROUP_BEGIN) {
            if (p.n_edges != 0u || p.lerp != 0u) bad("GROUP_BEGIN: n_edges and lerp must be 0");
            const int need = any_mask && masked[i] ? 2 : 1;
            if (levels + need > SWFR_MAX_LAYER_DEPTH) bad("group markers nest deeper than SWFR_MAX_LAYER_DEPTH");
            levels += need;
            open[depth++] = i;
            seen[depth] = PixelRect{};
        } else if (p.kind == SWFR_PATH_GROUP_END) {
            if (!depth) bad("GROUP_END without a GROUP_BEGIN");
            const swfr_path& g = paths[open[--depth]];
            levels -= any_mask && masked[open[depth]] ? 2 : 1;
            if (p.n_edges != 0u || (p.lerp & 0xffu) != 0u || ((p.lerp >> 8) & 0xffffu) > max_op) bad("GROUP_END: n_edges and lerp bits 0..7 and 16..23 must be 0, the operator at most 8");
            if ((p.lerp >> 24) != 0u && any_mask && masked[open[depth]]) bad("GROUP_END: a fade on a group with a GROUP_MASK");
            if (p.x_min != g.x_min || p.y_min != g.y_min || p.x_max != g.x_max || p.y_max != g.y_max) bad("group markers: the rectangles of GROUP_BEGIN and GROUP_END differ");
            const PixelRect& u = seen[depth];
            if (((p.lerp >> 8) & 0xffu) == SWFR_OP_ALPHA && !u.empty() && (u.x0 < p.x_min || u.y0 < p.y_min || u.x1 > p.x_max || u.y1 > p.y_max))
                bad("an ALPHA group's rectangle must contain every path drawn on its parent surface before it");
            seen[depth].add(p.x_min, p.y_min, p.x_max, p.y_max);
        } else if (p.kind == SWFR_PATH_GROUP_MASK) {
            const swfr_path& g = paths[open[depth - 1]];                  // (inside a group: checked above)
            if (p.n_edges != 0u || p.lerp != 0u) bad("GROUP_MASK: n_edges and lerp must be 0");
            if (p.x_min != g.x_min || p.y_min != g.y_min || p.x_max != g.x_max || p.y_max != g.y_max) bad("group markers: the rectangles of GROUP_BEGIN and GROUP_MASK differ");
            seen[depth] = PixelRect{};                                   // (the mask's surface starts clear)
        } else seen[depth].add(p.x_min, p.y_min, p.x_max, p.y_max);
    }
    if (depth) bad("GROUP_BEGIN without a GROUP_END");
}

// What the device sees of isolated groups ("Isolated layers").  A marker becomes a box path of ONE box, its rectangle, with
// a transparent solid style and lerp 0: to k2_bin and the row kernels an ordinary path that reaches exactly the strips of the
// rectangle, in painter's order, and paints nothing.  What it means travels in the path's operator byte (bits 8..15 of `lerp`, split off
// into Frame2::path_op by push_scene), which only k2_tiles<3> to <6> read: PATH_OP_GROUP_BEGIN, or PATH_OP_GROUP_END | operator
// (SWFR_PATH_GROUP_MASK: PATH_OP_GROUP_BEGIN | PATH_OP_MASKED, and its group's END carries PATH_OP_MASKED, too: k2_tiles<5>).  A
// path INSIDE a group loses its lerp bit (so that no kernel derives an opaque cover or a culling record from it: a cover inside a group
// hides nothing outside) and carries it in PATH_OP_LERP instead, where k2_tiles<4> reads it back for the pixel arithmetic.
// A FADED END (bits 24..31 of its lerp, swfr.h) carries PATH_OP_MASKED as well -- "a step before the composite" -- and, instead of the
// shared transparent style, one of its own whose `pixel` is the fade: the word k2_bin copies into the band entry (BandEntry2::solid),
// which the walk of k2_tiles holds as a scalar anyway.  Its alpha byte is 0: no kernel takes it for an opaque cover.  A masked END's
// solid word is 0, a faded END's is not: that tells the two steps apart (upload refuses a fade on a masked group).  `faded` says
// whether the scene has such an END: layout_scene then picks k2_tiles<6>.
// Returns false when the scene has no marker (nothing is copied).
bool lower_groups(const SceneView& sv, std::vector<swfr_edge>& out_e, std::vector<swfr_path>& out_p, std::vector<swfr_style>& out_s, bool& faded) {
    const auto [edges, n_edges, paths, n_paths, styles, n_styles] = sv;
    faded = false;
    bool any = false;
    for (size_t i = 0; i < n_paths && !any; ++i) any = paths[i].kind >= SWFR_PATH_GROUP_BEGIN;
    if (!any) return false;
    out_e.assign(edges, edges + n_edges); out_p.assign(paths, paths + n_paths); out_s.assign(styles, styles + n_styles);
    swfr_style clear;
    std::memset(&clear, 0, sizeof clear);
    clear.kind = SWFR_STYLE_SOLID;
    out_s.push_back(clear);
    uint32_t fade_style[256] = {0u};                             // the style of a fade value, once it has one (0: none yet): at most 255 more styles
    // (a MASK is to the device a second BEGIN, flagged PATH_OP_MASKED, and the END of its group pops both: it carries the flag, too)
    int depth = 0;
    uint32_t masked = 0u;                                        // bit d: the group open at depth d + 1 has had its MASK
    for (size_t i = 0; i < n_paths; ++i) {
        swfr_path& p = out_p[i];
        if (p.kind < SWFR_PATH_GROUP_BEGIN) {
            if (depth) p.lerp = ((p.lerp >> 8) | ((p.lerp & 1u) ? PATH_OP_LERP : 0u)) << 8;
            continue;
        }
        uint32_t fade = 0u;
        if (p.kind == SWFR_PATH_GROUP_MASK) {
            masked |= 1u << (depth - 1);
            p.lerp = (PATH_OP_GROUP_BEGIN | PATH_OP_MASKED) << 8;
        } else if (p.kind == SWFR_PATH_GROUP_END) {
            --depth;
            fade = p.lerp >> 24;
            p.lerp = (PATH_OP_GROUP_END | ((p.lerp >> 8) & PATH_OP_MASK) | (((masked >> depth) & 1u) || fade ? PATH_OP_MASKED : 0u)) << 8;
            masked &= ~(1u << depth);
        } else {
            ++depth;
            p.lerp = PATH_OP_GROUP_BEGIN << 8;
        }
        p.kind = SWFR_PATH_BOXES; p.fill_rule = 0; p.style = uint32_t(n_styles);
        if (fade) {
            faded = true;
            if (!fade_style[fade]) {
                swfr_style st = clear;
                st.pixel = fade;
                fade_style[fade] = uint32_t(out_s.size());
                out_s.push_back(st);
            }
            p.style = fade_style[fade];
        }
        p.first_edge = uint32_t(out_e.size()); p.n_edges = 1;
        swfr_edge b;
        std::memset(&b, 0, sizeof b);
        b.x1 = p.x_min * 256; b.y1 = p.y_min * 256; b.x2 = p.x_max * 256; b.y2 = p.y_max * 256;
        b.top = b.y1; b.bottom = b.y2; b.dir = 1; b.reserved = int32_t(i);
        out_e.push_back(b);
    }
    return true;
}

// swfr_style::extend of a gradient style: 0 pad, 1 repeat, 2 reflect; a linear gradient -- the float64 extension -- pads only
void validate_gradient_extend(const SceneView& sv) {
    for (size_t i = 0; i < sv.n_styles; ++i) {
        const swfr_style& s = sv.styles[i];
        if (s.kind != SWFR_STYLE_RADIAL && s.kind != SWFR_STYLE_LINEAR && s.kind != SWFR_STYLE_LINEAR_PIXMAN) continue;
        if (s.extend > 2) throw StatusError{SWFR_ERR_INVALID, "gradient extend must be 0 (pad), 1 (repeat) or 2 (reflect)"};
        if (s.kind == SWFR_STYLE_LINEAR && s.extend) throw StatusError{SWFR_ERR_NOT_IMPLEMENTED, "NotImplementedGradientSpread"};
    }
}

// swfr_style::filter of a bitmap style: 0 CAIRO_FILTER_GOOD, 1 CAIRO_FILTER_NEAREST; every other kind ignores the field
void validate_bitmap_filter(const SceneView& sv) {
    for (size_t i = 0; i < sv.n_styles; ++i)
        if (sv.styles[i].kind == SWFR_STYLE_BITMAP && sv.styles[i].filter > 1) throw StatusError{SWFR_ERR_INVALID, "bitmap filter must be 0 (good) or 1 (nearest)"};
}

// Validate a caller-supplied scene so that no kernel can index out of bounds.
// blur_ok: the scene is a frame swfr_render is drawing, whose blurred layers' textures (BLUR_BASE + k) have been made
void validate_scene(const swfr_renderer* r, const SceneView& sv, bool blur_ok = false) {
    const auto [edges, n_edges, paths, n_paths, styles, n_styles] = sv;
    // end points within +-32768 px (2^23 in 24.8): inside that range the int64 products of the closed-form edge evaluation cannot overflow
    for (size_t i = 0; i < n_edges; ++i) {
        const swfr_edge& e = edges[i];
        const int32_t lim = 1 << 23;
        if (e.x1 < -lim || e.x1 > lim || e.x2 < -lim || e.x2 > lim || e.y1 < -lim || e.y1 > lim || e.y2 < -lim || e.y2 > lim)
            throw StatusError{SWFR_ERR_INVALID, "edge end point outside +-32768 px"};
    }
    // every edge belongs to exactly one path: the paths' edge ranges are disjoint and cover the edge list (the kernels and the host
    // layout index the path table with the edge's owner)
    {
        static thread_local std::vector<uint8_t> owned;
        owned.assign(n_edges, 0);
        for (size_t i = 0; i < n_paths; ++i) {
            const swfr_path& p = paths[i];
            if (size_t(p.first_edge) + p.n_edges > n_edges) throw StatusError{SWFR_ERR_INVALID, "path edge range out of bounds"};
            for (size_t k = 0; k < p.n_edges; ++k) {
                if (owned[p.first_edge + k]) throw StatusError{SWFR_ERR_INVALID, "paths share an edge (their edge ranges overlap)"};
                owned[p.first_edge + k] = 1;
            }
        }
        for (size_t i = 0; i < n_edges; ++i)
            if (!owned[i]) throw StatusError{SWFR_ERR_INVALID, "an edge belongs to no path"};
    }
    for (size_t i = 0; i < n_paths; ++i) {
        const swfr_path& p = paths[i];
        if (size_t(p.first_edge) + p.n_edges > n_edges) throw StatusError{SWFR_ERR_INVALID, "path edge range out of bounds"};
        if (p.style >= n_styles && p.kind < SWFR_PATH_GROUP_BEGIN) throw StatusError{SWFR_ERR_INVALID, "path style index out of bounds"};
        if (p.kind > SWFR_PATH_GROUP_MASK) throw StatusError{SWFR_ERR_INVALID, "unknown path kind"};
        if (p.kind == SWFR_PATH_TOR)
            // an edge of the scan converter: a line (x1, y1)-(x2, y2) running downwards, active over [top, bottom) INSIDE its own extent
            // (what the frame builder and Cairo's clipper produce); the per-row stepping of k2_rows is exact only there
            for (size_t k = 0; k < p.n_edges; ++k) {
                const swfr_edge& e = edges[p.first_edge + k];
                if (e.top >= e.bottom) continue;                              // never active
                if (!(e.y1 < e.y2 && e.y1 <= e.top && e.bottom <= e.y2))
                    throw StatusError{SWFR_ERR_INVALID, "edge active outside its line: need y1 < y2 and y1 <= top < bottom <= y2"};
            }
        if (p.x_min < 0 || p.y_min < 0 || p.x_max > int(r->width) || p.y_max > int(r->height) || p.x_min > p.x_max || p.y_min > p.y_max)
            throw StatusError{SWFR_ERR_INVALID, "path pixel rectangle outside the frame"};
    }
    for (size_t i = 0; i < n_styles; ++i) {
        const swfr_style& s = styles[i];
        if (s.kind > SWFR_STYLE_LINEAR_PIXMAN) throw StatusError{SWFR_ERR_INVALID, "unknown style kind"};
        if (s.n_stops > SWFR_MAX_STOPS) throw StatusError{SWFR_ERR_INVALID, "too many gradient stops"};
        if (s.kind == SWFR_STYLE_LINEAR_PIXMAN) {
            // aliased, libcairo composites span by span and pixman starts the ramp anew at every span: the tile pass does not have the
            // start of a covered run that begins left of its strip, so the combination is refused, never approximated
            if (r->mono) throw StatusError{SWFR_ERR_NOT_IMPLEMENTED, "NotImplementedAliasedPixmanLinear"};
            if (s.c0x == s.c1x && s.c0y == s.c1y) throw StatusError{SWFR_ERR_INVALID, "a pixman-linear gradient needs two distinct points (c0 == c1)"};
        }
        if (s.kind == SWFR_STYLE_BITMAP) {
            const auto& V = r->builder->variants();
            const bool known = s.bitmap >= BLUR_BASE ? (blur_ok && s.bitmap - BLUR_BASE < r->blur_table.size() && r->blur_table[s.bitmap - BLUR_BASE].pixels != nullptr)
                               : s.bitmap >= VARIANT_BASE ? (s.bitmap - VARIANT_BASE < V.size() && r->bitmaps.count(V[s.bitmap - VARIANT_BASE].bitmap))
                                                        : r->bitmaps.count(s.bitmap) != 0;
            if (!known) throw StatusError{SWFR_ERR_NOT_FOUND, "BitmapNotFound"};
        }
    }
}

// CAIRO_FILTER_GOOD for a surface pattern (cairo-pattern.c _cairo_pattern_analyze_filter, cairo-image-source.c
// create_separable_convolution): bilinear unless an axis is minified below 0.75; then a box (x) tent kernel per axis,
// sampled at 2^bits phases, weights in 16.16, normalised with the rounding error put on the centre tap.
double good_box_kernel(double x, double r) { return std::max(0.0, std::min(std::min(r, 1.0), std::min((r + 1) / 2 - x, (r + 1) / 2 + x))); }
void good_axis(double r, int& width, int& bits, std::vector<int32_t>& out) {
    width = r < 1.0 ? 2 : int(std::ceil(r + 1));
    bits = 0;
    if (width > 1) while (r * double(1 << bits) <= 128.0) ++bits;
    const int n_phases = 1 << bits;
    const double step = 1.0 / n_phases;
    for (int i = 0; i < n_phases; ++i) {
        const size_t base = out.size();
        if (width <= 1) { out.push_back(65536); continue; }
        const double frac = (i + .5) * step;
        const double x1 = std::ceil(frac - width / 2.0 - 0.5) - frac + 0.5;   // centre of the left-most tap
        double total = 0;
        for (int j = 0; j < width; ++j) { const double v = good_box_kernel(x1 + j, r); total += v; out.push_back(int32_t(v * 65536.0)); }
        total = 1 / total;
        int32_t new_total = 0;
        for (int j = 0; j < width; ++j) new_total += (out[base + size_t(j)] = int32_t(out[base + size_t(j)] * total));
        out[base + size_t(width / 2)] += 65536 - new_total;
    }
}
bool good_use_bilinear(double x, double y, double t) {
    const double h = x * x + y * y;                                   // device -> pattern matrix row
    if (h < 1.0 / (0.75 * 0.75)) return true;
    if (h > 3.99 && h < 4.01 && to_fixed(x * y) == 0 && (to_fixed(t) & 255) == 0) return true;   // exactly 1/2, axis-parallel, integer offset
    return false;
}
int64_t fixed_16_16(double d) { return int64_t(std::nearbyint(d * 65536.0)); }   // _cairo_fixed_16_16_from_double: ties to even

// The pattern matrix as pixman gets it (cairo-matrix.c _cairo_matrix_to_pixman_matrix_offset, cairo-image-source.c
// _pixman_image_set_properties): an integer translation is split off so that what remains is small, the matrix is rounded to
// 16.16 and its translation is corrected until the centre of the operation's rectangle maps where the double matrix puts it.
struct PixmanPosition { int64_t base_x, base_y; int32_t m00, m01, m10, m11; };
PixmanPosition pixman_transform_of(Affine m, const int rect[4]) {
    PixmanPosition f;
    const double xc = rect[0] + (rect[2] - rect[0]) / 2., yc = rect[1] + (rect[3] - rect[1]) / 2.;
    int64_t ox = 0, oy = 0;
    if (m.x0 != 0.0 || m.y0 != 0.0) {
        double tx = m.x0, ty = m.y0, norm = std::max(std::fabs(tx), std::fabs(ty));
        for (int i = -1; i < 2; i += 2)
            for (int j = -1; j < 2; j += 2) {
                double den = (m.xx + i) * (m.yy + j) - m.xy * m.yx;
                if (std::fabs(den) < DBL_EPSILON) continue;
                double x = m.y0 * m.xy - m.x0 * (m.yy + j), y = m.x0 * m.yx - m.y0 * (m.xx + i);
                den = 1 / den;
                x *= den;
                y *= den;
                const double new_norm = std::max(std::fabs(x), std::fabs(y));
                if (norm > new_norm) { norm = new_norm; tx = x; ty = y; }
            }
        tx = std::floor(tx);
        ty = std::floor(ty);
        ox = int64_t(-tx);
        oy = int64_t(-ty);
        Affine t;
        t.x0 = tx; t.y0 = ty;
        m = t.then(m);                                              // cairo_matrix_translate
    }
    int64_t p[2][3] = {{fixed_16_16(m.xx), fixed_16_16(m.xy), fixed_16_16(m.x0)}, {fixed_16_16(m.yx), fixed_16_16(m.yy), fixed_16_16(m.y0)}};
    const double eps = 1.0 / 256.0, det = m.det();
    const bool unity = std::fabs(det * det - 1.0) < eps &&
                       ((std::fabs(m.xy) < eps && std::fabs(m.yx) < eps) || (std::fabs(m.xx) < eps && std::fabs(m.yy) < eps));
    Affine inv = m;
    if (!unity && inv.invert_cairo()) {
        for (int it = 0; it < 5; ++it) {
            const int64_t vx = fixed_16_16(xc), vy = fixed_16_16(yc);
            const int64_t tx = (p[0][0] * vx + p[0][1] * vy + p[0][2] * 65536 + 0x8000) >> 16;
            const int64_t ty = (p[1][0] * vx + p[1][1] * vy + p[1][2] * 65536 + 0x8000) >> 16;
            // pixman_transform_point_3d fails when the centre does not map into 16.16 (|coordinate| >= 32768): Cairo then leaves
            // the translation as rounded ("If we can't transform the reference point, skip the adjustment")
            if (tx != (int32_t)tx || ty != (int32_t)ty) break;
            double x = double(tx) / 65536.0, y = double(ty) / 65536.0;
            inv.apply(x, y);
            x -= xc;
            y -= yc;
            m.apply_distance(x, y);
            const int64_t dx = fixed_16_16(x), dy = fixed_16_16(y);
            p[0][2] -= dx;
            p[1][2] -= dy;
            if (dx == 0 && dy == 0) break;
        }
    }
    // pixman_transform_point_3d of pixel (px, py)'s centre: (p·(X, Y, 1) + 0x8000) >> 16 with X = (px + ox + .5) in 16.16; the
    // per-pixel and per-row steps are whole multiples of 65536 inside the sum, so they come out of the shift exactly
    const int64_t X0 = ox * 65536 + 0x8000, Y0 = oy * 65536 + 0x8000;
    f.base_x = (p[0][0] * X0 + p[0][1] * Y0 + p[0][2] * 65536 + 0x8000) >> 16;
    f.base_y = (p[1][0] * X0 + p[1][1] * Y0 + p[1][2] * 65536 + 0x8000) >> 16;
    f.m00 = int32_t(p[0][0]); f.m01 = int32_t(p[0][1]); f.m10 = int32_t(p[1][0]); f.m11 = int32_t(p[1][1]);
    return f;
}
Affine pattern_matrix(const swfr_style& st) {
    Affine m;
    m.xx = st.inv[0]; m.yx = st.inv[1]; m.xy = st.inv[2]; m.yy = st.inv[3]; m.x0 = st.inv[4]; m.y0 = st.inv[5];
    return m;
}

// A radial gradient as cairo 1.16 hands it to pixman 0.40 and as pixman evaluates it: circles scaled into +-16383 (the matrix
// takes the inverse factor), 16.16 circles and stops, 16-bit colours, single-precision ramps per interval (gradient_walker_reset),
// PAD sentinels.  The device evaluates B and C of the quadratic as exact 64-bit integers, the root in doubles, the ramp in floats.
// Under REPEAT or REFLECT (swfr_style::extend 1, 2) the ramp of an interval depends on the period the position lies in -- pixman
// forms it in single precision from the interval's ends shifted into that period -- so no table can hold it: the device gets the
// 16.16 stops with the sentinels of the repeat kind, the 16-bit colours and the left edge of the operation's rectangle, where
// pixman starts a scanline's walker, and resets per pixel (raster_common.hip, shade_spread).
void gradient_stops_of(const swfr_style& st, const int rect[4], DevGradient& g);
DevGradient radial_of(const swfr_style& st, const int rect[4]) {
    DevGradient g;
    std::memset(&g, 0, sizeof g);
    double c0x = st.c0x, c0y = st.c0y, c0r = st.r0, c1x = st.c1x, c1y = st.c1y, c1r = st.r1;
    double dim = std::fabs(c0x);
    for (double v : {c0y, c0r, c1x, c1y, c1r, c0x - c1x, c0y - c1y, c0r - c1r}) dim = std::max(dim, std::fabs(v));
    Affine m = pattern_matrix(st);
    if (dim > 16383.0) {                                            // PIXMAN_MAX_INT >> 1
        dim = 16383.0 / dim;
        c0x *= dim; c0y *= dim; c0r *= dim; c1x *= dim; c1y *= dim; c1r *= dim;
        m = m.then(Affine::scale(dim, dim));
    }
    const PixmanPosition pos = pixman_transform_of(m, rect);
    g.base_x = pos.base_x; g.base_y = pos.base_y; g.m00 = pos.m00; g.m01 = pos.m01; g.m10 = pos.m10; g.m11 = pos.m11;
    const int64_t f1x = fixed_16_16(c0x), f1y = fixed_16_16(c0y), f1r = fixed_16_16(c0r);
    const int64_t dx = fixed_16_16(c1x) - f1x, dy = fixed_16_16(c1y) - f1y, dr = fixed_16_16(c1r) - f1r;
    g.c1x = int32_t(f1x); g.c1y = int32_t(f1y); g.c1r = int32_t(f1r); g.dx = int32_t(dx); g.dy = int32_t(dy); g.dr = int32_t(dr);
    g.a = double(dx * dx + dy * dy - dr * dr);
    g.inva = g.a != 0 ? 1. * 65536 / g.a : 0;
    g.mindr = -1. * 65536 * double(f1r);
    gradient_stops_of(st, rect, g);
    return g;
}
// The walker's part of a DevGradient, the same for a radial and a pixman-linear style: 16.16 stops, 16-bit colours, the sentinels of
// the extend, and the ramp table (pad) or the colours and the rectangle's left edge (repeat, reflect)
void gradient_stops_of(const swfr_style& st, const int rect[4], DevGradient& g) {
    const int n = int(st.n_stops);
    g.n_intervals = n ? n + 1 : 0;
    uint16_t col[SWFR_MAX_STOPS + 2][4] = {};
    for (int i = 0; i < n; ++i) {
        g.x[i + 1] = int32_t(fixed_16_16(double(st.stop_offset[i])));
        // cairo_pattern_add_color_stop_rgba keeps doubles; _cairo_color_double_to_short = (uint16)(v * 65535 + 0.5)
        col[i + 1][0] = uint16_t(double(st.stop_rgba[i][3]) * 65535.0 + 0.5);
        col[i + 1][1] = uint16_t(double(st.stop_rgba[i][0]) * 65535.0 + 0.5);
        col[i + 1][2] = uint16_t(double(st.stop_rgba[i][1]) * 65535.0 + 0.5);
        col[i + 1][3] = uint16_t(double(st.stop_rgba[i][2]) * 65535.0 + 0.5);
    }
    g.x[0] = INT32_MIN; g.x[n + 1] = INT32_MAX;
    if (n) { std::memcpy(col[0], col[1], sizeof col[0]); std::memcpy(col[n + 1], col[n], sizeof col[0]); }
    if (st.extend && n) {
        // _pixman_gradient_walker_init's sentinel stops: REPEAT -- the last stop one period down, the first one period up;
        // REFLECT -- the first stop mirrored at 0, the last mirrored at 1
        g.extend = int32_t(st.extend); g.x_min = rect[0];
        if (st.extend == 1) {
            g.x[0] = g.x[n] - 0x10000; g.x[n + 1] = g.x[1] + 0x10000;
            std::memcpy(col[0], col[n], sizeof col[0]); std::memcpy(col[n + 1], col[1], sizeof col[0]);
        } else {
            g.x[0] = -g.x[1]; g.x[n + 1] = 0x20000 - g.x[n];
        }
        std::memcpy(g.col, col, sizeof col);
        return;
    }
    for (int k = 0; k <= n && n; ++k) {
        const int64_t left_x = g.x[k], right_x = g.x[k + 1];
        const float lx = left_x * (1.0f / 65536.0f), rx = right_x * (1.0f / 65536.0f);
        for (int ch = 0; ch < 4; ++ch) {
            const float l = col[k][ch] * (1.0f / 257.0f), rr = col[k + 1][ch] * (1.0f / 257.0f);
            if ((-FLT_MIN < (rx - lx) && (rx - lx) < FLT_MIN) || left_x == INT32_MIN || right_x == INT32_MAX) {
                g.ramp[k][2 * ch] = 0.0f;
                g.ramp[k][2 * ch + 1] = (l + rr) / 510.0f;
            } else {
                const float w_rec = 1.0f / (rx - lx);
                g.ramp[k][2 * ch + 1] = (l * rx - rr * lx) * w_rec * (1.0f / 255.0f);
                g.ramp[k][2 * ch] = (rr - l) * w_rec * (1.0f / 255.0f);
            }
        }
    }
}

// A linear gradient as cairo 1.16 hands it to pixman 0.40 and as pixman evaluates it (pixman-linear-gradient.c, linear_get_scanline,
// the affine branch): the end points scaled into +-16383 (the matrix takes the inverse factor), 16.16 points, and per scanline of a
// PIECE -- what libcairo hands to pixman_image_composite32 as one rectangle -- with v the 16.16 sample position at the piece's left edge
//     t = ((double)(dx v.x + dy v.y) - (double)(dx p1.x + dy p1.y)) * invden,  invden = 65536 / (double)(dx^2 + dy^2)
//     inc = (double)(dx m00 + dy m10) * invden,   position of the i-th pixel of the piece = trunc(t) + trunc(inc * i)
// The fields of the radial record are reused: c1x, c1y = p1; dx, dy; a = (double)(dx p1.x + dy p1.y); inva = invden; mindr = inc;
// x_min = the rectangle's left edge (the origin of a box path's one piece); pad, c1r, dr: the table of piece origins of a tor
// path -- offset + 1 into the handle's int32 table (0: none), the rectangle's first row, entries per row (prepare_sources).
// Refused, never approximated: a rectangle whose corner pixels (it grown by one pixel, as pixman's analyze_extent grows it) leave
// 16.16 -- libcairo then paints some rows or none -- and a position that moves by less than one 16.16 unit per pixel row without
// standing still: pixman then evaluates the first scanline of a piece for all its rows (linear_gradient_is_horizontal), and which
// rows libcairo gathers into one piece the tile pass does not know.
DevGradient linear_of(const swfr_style& st, const int rect[4]) {
    DevGradient g;
    std::memset(&g, 0, sizeof g);
    double x1 = st.c0x, y1 = st.c0y, x2 = st.c1x, y2 = st.c1y;
    double dim = std::fabs(x1);
    for (double v : {y1, x2, y2, x1 - x2, y1 - y2}) dim = std::max(dim, std::fabs(v));
    Affine m = pattern_matrix(st);
    if (dim > 16383.0) {                                            // _cairo_gradient_pattern_fit_to_range, PIXMAN_MAX_INT >> 1
        dim = 16383.0 / dim;
        x1 *= dim; y1 *= dim; x2 *= dim; y2 *= dim;
        m = m.then(Affine::scale(dim, dim));
    }
    const PixmanPosition pos = pixman_transform_of(m, rect);
    g.base_x = pos.base_x; g.base_y = pos.base_y; g.m00 = pos.m00; g.m01 = pos.m01; g.m10 = pos.m10; g.m11 = pos.m11;
    const int64_t p1x = fixed_16_16(x1), p1y = fixed_16_16(y1), dx = fixed_16_16(x2) - p1x, dy = fixed_16_16(y2) - p1y;
    const int64_t l = dx * dx + dy * dy;
    if (l == 0) throw StatusError{SWFR_ERR_INVALID, "a pixman-linear gradient needs two distinct points (c0 == c1 in 16.16)"};
    for (int px : {rect[0] - 1, rect[2]})
        for (int py : {rect[1] - 1, rect[3]}) {
            const int64_t vx = pos.base_x + int64_t(px) * pos.m00 + int64_t(py) * pos.m01, vy = pos.base_y + int64_t(px) * pos.m10 + int64_t(py) * pos.m11;
            const int64_t lim = (int64_t(1) << 31) - 8;
            if (vx < -lim || vx >= lim || vy < -lim || vy >= lim) throw StatusError{SWFR_ERR_CAPACITY, "LinearGradientOutOfRange"};
        }
    g.c1x = int32_t(p1x); g.c1y = int32_t(p1y); g.dx = int32_t(dx); g.dy = int32_t(dy);
    g.a = double(dx * p1x + dy * p1y);
    g.inva = 65536.0 * 65536.0 / (double(l) * 65536.0);
    g.mindr = double(dx * pos.m00 + dy * pos.m10) * g.inva;
    const double row_step = double(dx * pos.m01 + dy * pos.m11) * g.inva;
    if (row_step != 0 && row_step > -1 && row_step < 1) throw StatusError{SWFR_ERR_NOT_IMPLEMENTED, "NotImplementedLinearRowStep"};
    gradient_stops_of(st, rect, g);
    g.extend = int32_t(st.extend); g.x_min = rect[0]; g.pad = 0;
    return g;
}

DevFilter good_filter(const swfr_style& st, const int rect[4], std::vector<int32_t>& params) {
    DevFilter f{};
    if (st.kind != SWFR_STYLE_BITMAP) return f;
    const PixmanPosition pos = pixman_transform_of(pattern_matrix(st), rect);
    f.base_x = pos.base_x; f.base_y = pos.base_y; f.m00 = pos.m00; f.m01 = pos.m01; f.m10 = pos.m10; f.m11 = pos.m11;
    // CAIRO_FILTER_NEAREST: one texel at every scale -- no convolution however small the scale (`on` stays 0) -- fetched by the bilinear
    // routes with their weights masked to zero; their "half a texel back" must land pixman_fixed_e back, so the base moves by the rest
    if (st.filter == 1) { f.nearest = 1; f.base_x += 0x8000 - 1; f.base_y += 0x8000 - 1; return f; }
    const double xx = st.inv[0], yx = st.inv[1], xy = st.inv[2], yy = st.inv[3], x0 = st.inv[4], y0 = st.inv[5];
    if (good_use_bilinear(xx, xy, x0) && good_use_bilinear(yx, yy, y0)) return f;
    double dx = std::hypot(xx, xy), dy = std::hypot(yx, yy);
    dx = std::min(dx, 16.0); dy = std::min(dy, 16.0);
    if (dx < 1.0 / 0.75) dx = 1.0;
    if (dy < 1.0 / 0.75) dy = 1.0;
    f.on = 1;
    f.x_off = uint32_t(params.size());
    good_axis(dx, f.cw, f.xbits, params);
    f.y_off = uint32_t(params.size());
    good_axis(dy, f.ch, f.ybits, params);
    return f;
}

// pixman's view of every bitmap / radial-gradient style of a scene (sample positions, filter tables, colour ramps)
constexpr int LINEAR_RUN_LENGTH = 256;      // cairo-image-compositor.c, inplace_renderer_init: run_length of a linear or radial source
// sv: the scene as drawn (the edges of a pixman-linear box path are looked at); split: the device gets column blocks of its paths
// (split_wide_paths); n_linear: how many pixman-linear styles got a table of piece origins for k2_linear_pieces to fill
void prepare_sources(const SceneView& sv, bool split, size_t& n_linear, std::vector<DevFilter>& filters, std::vector<DevGradient>& gradients,
                     std::vector<int32_t>& fparams, const std::vector<DevBitmap>& bitmap_table, const std::vector<DevBitmap>& variant_table,
                     const std::vector<DevBitmap>& blur_table) {
    const auto [edges, n_edges, paths, n_paths, styles, n_styles] = sv;
    filters.assign(n_styles, DevFilter{});
    // a bitmap style belongs to one drawing operation: pixman's transform is anchored at the centre of that operation's rectangle
    std::vector<int> rect(4 * n_styles, 0);
    std::vector<uint8_t> seen(n_styles, 0);
    std::vector<uint32_t> owner(n_styles, ~0u);                   // the one path of a pixman-linear style
    n_linear = 0;
    for (size_t i = 0; i < n_paths; ++i) {
        const swfr_path& p = paths[i];
        if (styles[p.style].kind != SWFR_STYLE_BITMAP && styles[p.style].kind != SWFR_STYLE_RADIAL && styles[p.style].kind != SWFR_STYLE_LINEAR_PIXMAN) continue;
        if (styles[p.style].kind == SWFR_STYLE_LINEAR_PIXMAN) {
            // libcairo starts the ramp anew at every piece it composites: one path per style, and of a rectilinear path only what is
            // one piece -- a single box, on whole pixels or no wider than the run length at which libcairo's span renderer splits a row
            if (seen[p.style]) throw StatusError{SWFR_ERR_INVALID, "a pixman-linear gradient style belongs to one path"};
            if (split) throw StatusError{SWFR_ERR_CAPACITY, "a pixman-linear gradient on a path wider than 8192 px"};
            if (p.kind == SWFR_PATH_BOXES) {
                bool whole = true;
                if (p.n_edges == 1 && edges) { const swfr_edge& b = edges[p.first_edge]; whole = !((b.x1 | b.x2 | b.y1 | b.y2) & 255); }
                if (p.n_edges > 1 || (!whole && p.x_max - p.x_min > LINEAR_RUN_LENGTH)) throw StatusError{SWFR_ERR_NOT_IMPLEMENTED, "NotImplementedLinearPieces"};
            }
            owner[p.style] = uint32_t(i);
        }
        int* q = &rect[4 * size_t(p.style)];
        if (seen[p.style] && (q[0] != p.x_min || q[1] != p.y_min || q[2] != p.x_max || q[3] != p.y_max))
            throw StatusError{SWFR_ERR_INVALID, "paths that share a bitmap or radial-gradient style must share the pixel rectangle (one drawing operation)"};
        seen[p.style] = 1;
        q[0] = p.x_min; q[1] = p.y_min; q[2] = p.x_max; q[3] = p.y_max;
    }
    for (size_t i = 0; i < n_styles; ++i) {
        filters[i] = good_filter(styles[i], &rect[4 * i], fparams);
        filters[i].kind = styles[i].kind; filters[i].extend = styles[i].extend;
        if (styles[i].kind == SWFR_STYLE_BITMAP) {
            // (a colour-transformed bitmap samples its texture from the texel pass: resolve_variants)
            const uint32_t b = styles[i].bitmap;
            const DevBitmap* bm = b >= BLUR_BASE ? (b - BLUR_BASE < blur_table.size() ? &blur_table[b - BLUR_BASE] : nullptr)
                                  : b >= VARIANT_BASE ? (b - VARIANT_BASE < variant_table.size() ? &variant_table[b - VARIANT_BASE] : nullptr)
                                                    : (b < bitmap_table.size() ? &bitmap_table[b] : nullptr);
            if (bm) { filters[i].pixels = bm->pixels; filters[i].width = bm->width; filters[i].height = bm->height; }
        }
        if (styles[i].kind == SWFR_STYLE_RADIAL) {
            gradients.push_back(radial_of(styles[i], &rect[4 * i]));
            filters[i].pad = int32_t(gradients.size());            // index + 1 into the gradient table
        }
        if (styles[i].kind == SWFR_STYLE_LINEAR_PIXMAN) {
            const int* q = &rect[4 * i];
            DevGradient g = linear_of(styles[i], q);
            if (owner[i] != ~0u && paths[owner[i]].kind == SWFR_PATH_TOR && q[2] > q[0] && q[3] > q[1]) {
                // a tor path: libcairo's span renderer composites every row in pieces of its own (cairo-image-compositor.c,
                // _inplace_spans: from the row's first span on, cut at runs of 256 and more full or empty pixels), which only the
                // row pass's cells tell.  k2_linear_pieces writes the pieces' first columns here, per row, per frame -- the same
                // values every frame: they follow from the scene alone.  Header: the path, then `per_row` columns a row, ascending,
                // INT32_MAX behind the last; none: the rectangle's left edge
                const int per_row = 2 * ((q[2] - q[0]) / LINEAR_RUN_LENGTH) + 2;
                fparams.push_back(int32_t(owner[i]));
                g.pad = int32_t(fparams.size()) + 1; g.c1r = q[1]; g.dr = per_row;
                fparams.resize(fparams.size() + size_t(per_row) * size_t(q[3] - q[1]), INT32_MAX);
                ++n_linear;
            }
            gradients.push_back(g);
            filters[i].pad = int32_t(gradients.size());
        }
    }
}

// What the host works out about a scene: the LAYOUT of the tables the device fills -- how many row chunks, band
// entries and cells there can be and where each path's share starts (prefix sums over the paths' rectangles and edge row spans,
// and over the tile-rows) -- plus pixman's view of the bitmap / gradient styles.  No binning: that is the device's work, per frame.
struct SceneLayout {
    uint32_t chunk_rows = ROWS_CHUNK;
    size_t n_chunks = 0, n_slots = 0, n_rows = 0, n_bands = 0, n_strips = 0, n_strip_slots = 0, incidences = 0, cell_main = 0, cell_total = 0;
    uint32_t max_path_edges = 0;
    bool rows_wide = false;     // the row kernel's wide instance although no path has more than ROWS_STAGE edges (SWFR_ROWS_WIDE)
    int shader_level = 0;       // 0 solid colours only, 1 + bitmap fills, 2 + gradients, 3 + blend operators, 4 + isolated groups, 5 + masked groups, 6 + faded groups, 7 + the erase and alpha operators: picks the tile kernel's instance
    bool any_blend = false;     // some path carries an operator byte (swfr_path::lerp >> 8; lower_groups): the arena gets the path_op table
    std::vector<uint32_t> chunk_base, slot_base, inc_base, band_off;
    std::vector<uint32_t> band_span;     // per path: first tile-row | last tile-row << 16 of its rectangle (0xffff | 0 << 16: none); padded to a multiple of 16 paths
    std::vector<DevFilter> filters;
    std::vector<DevGradient> gradients;
    std::vector<int32_t> fparams;
    size_t n_linear = 0;        // pixman-linear styles on tor paths: k2_linear_pieces runs between the row pass and the tile pass (0: not launched)
};
// sv: the scene as the device gets it; its edges carry their path index in `reserved`
// drawn: the scene as the caller drew it, when sv holds the column blocks of wide paths (split_wide_paths): a bitmap or
// gradient style is anchored at the rectangle of its drawing operation, not of a block
void layout_scene(const swfr_renderer* r, const SceneView& sv, SceneLayout& L, const SceneView* drawn = nullptr, bool faded = false) {
    const swfr_edge* const edges = sv.edges; const swfr_path* const paths = sv.paths; const swfr_style* const styles = sv.styles;
    const size_t n_edges = sv.n_edges, n_paths = sv.n_paths, n_styles = sv.n_styles;
    L.n_bands = (r->height + TILE_H - 1) / TILE_H;
    const uint32_t tiles_x = (r->width + TILE_W - 1) / TILE_W;
    // rows per k2_rows wavefront: 64 when that already gives the GPU a thousand wavefronts, fewer (whole tile-rows) for scenes made
    // of a few tall paths
    auto count_chunks = [&](uint32_t cr) {
        size_t n = 0;
        for (size_t i = 0; i < n_paths; ++i)
            if (paths[i].kind == SWFR_PATH_TOR && paths[i].y_max > paths[i].y_min)
                n += (size_t(paths[i].y_max) - size_t(paths[i].y_min) / TILE_H * TILE_H + cr - 1) / cr;
        return n;
    };
    // (counted over the whole frame also for a handle that owns a share of the tile-rows: with chunks sized for the share alone
    //  -- 16 rows at an eighth of S1 -- k2_bin writes four times the chunk descriptors and loses what k2_rows gains:
    //  profiles/r03o_blocks_timing.json)
    L.chunk_rows = ROWS_CHUNK;
    // (down to the rows of ONE STRIP for a frame of a few tall paths: its row kernel is as slow as its slowest wavefront, and a wavefront
    //  whose rows all need sample passes runs one pass per four rows)
    if (r->force_chunk_rows == 8 || r->force_chunk_rows == 16 || r->force_chunk_rows == 32 || r->force_chunk_rows == 64) L.chunk_rows = uint32_t(r->force_chunk_rows);
    else while (L.chunk_rows > uint32_t(STRIP_H) && count_chunks(L.chunk_rows) < 1024) L.chunk_rows >>= 1;
    L.shader_level = 0;
    for (size_t i = 0; i < n_styles; ++i)
        L.shader_level = std::max(L.shader_level, styles[i].kind == SWFR_STYLE_SOLID ? 0 : (styles[i].kind == SWFR_STYLE_BITMAP ? 1 : 2));
    uint32_t blend_bits = 0;
    bool alpha_ops = false;                                      // SWFR_OP_ERASE or SWFR_OP_ALPHA on a path or an END: the instance that has them
    for (size_t i = 0; i < n_paths; ++i) { blend_bits |= paths[i].lerp; alpha_ops = alpha_ops || ((paths[i].lerp >> 8) & PATH_OP_MASK) >= uint32_t(SWFR_OP_ERASE); }
    L.any_blend = (blend_bits >> 8) != 0u;
    if (L.any_blend) L.shader_level = (blend_bits >> 8) & PATH_OP_MASKED ? 5 : ((blend_bits >> 8) & (PATH_OP_GROUP_BEGIN | PATH_OP_GROUP_END) ? 4 : 3);
    if (faded) L.shader_level = 6;                               // (lower_groups met a faded END: the instance that fades)
    if (alpha_ops) L.shader_level = 7;                           // (instance 6 plus the two combiners and the ALPHA END rule)
    // (the test knobs: a higher instance than the frame needs -- with the style table in its full format -- and the wide row kernel)
    L.shader_level = std::max(L.shader_level, r->tiles_shaders);
    L.rows_wide = r->rows_wide;
    // exclusive prefixes over the paths (first chunk, first band slot) and over the tile-rows (band list offsets, by a difference
    // array over the paths' tile-row ranges)
    L.n_chunks = L.n_slots = L.n_rows = 0; L.max_path_edges = 0;
    L.chunk_base.assign(n_paths + 1, 0); L.slot_base.assign(n_paths + 1, 0); L.inc_base.assign(n_paths + 1, 0); L.band_off.assign(L.n_bands + 2, 0);
    L.band_span.assign((n_paths + 15) / 16 * 16 + 16, 0xffffu);
    for (size_t i = 0; i < n_paths; ++i) {
        const swfr_path& p = paths[i];
        L.chunk_base[i] = uint32_t(L.n_chunks); L.slot_base[i] = uint32_t(L.n_slots);
        if (p.kind == SWFR_PATH_TOR && p.x_max - p.x_min > MAX_PATH_WIDTH)
            throw StatusError{SWFR_ERR_CAPACITY, "a path wider than 8192 px reached the layout unsplit (cell columns are kept in 13 bits relative to the path)"};
        if (p.kind == SWFR_PATH_TOR && p.y_max > p.y_min) L.n_chunks += (size_t(p.y_max) - size_t(p.y_min) / TILE_H * TILE_H + L.chunk_rows - 1) / L.chunk_rows;
        if (p.y_max > p.y_min && p.x_max > p.x_min) {
            const size_t b0 = size_t(p.y_min / TILE_H), b1 = size_t((p.y_max - 1) / TILE_H);
            L.n_slots += b1 - b0 + 1;
            ++L.band_off[b0 + 1]; --L.band_off[b1 + 2];
            L.band_span[i] = uint32_t(b0) | (uint32_t(b1) << 16);
        }
        if (p.kind == SWFR_PATH_TOR) { L.n_rows += size_t(p.y_max - p.y_min); L.max_path_edges = std::max(L.max_path_edges, p.n_edges); }
    }
    L.chunk_base[n_paths] = uint32_t(L.n_chunks); L.slot_base[n_paths] = uint32_t(L.n_slots);
    for (size_t b = 1; b <= L.n_bands + 1; ++b) L.band_off[b] += L.band_off[b - 1];       // difference array -> counts, shifted by one
    for (size_t b = 1; b <= L.n_bands + 1; ++b) L.band_off[b] += L.band_off[b - 1];       // counts -> exclusive prefix: entries of tile-rows < b
    // pixel rows an edge can have a sample row in (a bound: +1 for the rounding of the sample grid): every (edge, row) pair yields
    // at most MAX_CELLS_PER_EDGE_ROW cells
    for (size_t i = 0; i < n_edges; ++i) {
        const swfr_edge& e = edges[i];
        const swfr_path& p = paths[e.reserved];
        if (p.kind != SWFR_PATH_TOR) continue;
        const int64_t top = std::max<int64_t>(e.top, int64_t(p.y_min) * 256), bot = std::min<int64_t>(e.bottom, int64_t(p.y_max) * 256);
        if (bot > top) L.inc_base[size_t(e.reserved) + 1] += uint32_t(((bot + 255) >> 8) - (top >> 8)) + 1;
    }
    for (size_t i = 0; i < n_paths; ++i) L.inc_base[i + 1] += L.inc_base[i];
    L.incidences = L.inc_base[n_paths];
    L.cell_main = L.incidences * MAX_CELLS_PER_EDGE_ROW;
    L.cell_total = L.cell_main * 2 + 4096;
    if (L.cell_total > 0xfffffff0ull) throw StatusError{SWFR_ERR_CAPACITY, "scene too large for 32-bit cell offsets"};
    L.n_strips = size_t(local_tile_rows(r)) * tiles_x * STRIPS_PER_TILE;
    L.n_strip_slots = strip_slots(local_tile_rows(r), uint32_t(tiles_x * STRIPS_PER_TILE));
    L.filters.clear(); L.gradients.clear(); L.fparams.clear();
    prepare_sources(drawn ? *drawn : sv, drawn != nullptr, L.n_linear, L.filters, L.gradients, L.fparams, r->bitmap_table, r->variant_table, r->blur_table);
}
// A tor path wider than the 13-bit column field of a cell (only possible in frames wider than 8192 px) is rasterized as several
// paths over the SAME edges, one per block of 8192 pixel columns: the scan converter clips a path's cells to its column range
// exactly the way a tile does -- a cell left of the range only adds its height to the range's first column, a cell right of it is
// dropped -- so the blocks' pixels are the pixels of the whole path, and the blocks do not overlap.  (A bitmap or gradient style stays
// anchored at the rectangle of the unsplit path: layout_scene gets the original paths for that.)  Returns false when the scene
// has no such path; otherwise the new edge list (tagged with the owning path) and path table.
bool split_wide_paths(const SceneView& sv, std::vector<swfr_edge>& out_e, std::vector<swfr_path>& out_p) {
    const swfr_edge* const edges = sv.edges; const swfr_path* const paths = sv.paths; const size_t n_paths = sv.n_paths;
    bool any = false;
    for (size_t i = 0; i < n_paths && !any; ++i) any = paths[i].kind == SWFR_PATH_TOR && paths[i].x_max - paths[i].x_min > MAX_PATH_WIDTH;
    if (!any) return false;
    out_e.clear(); out_p.clear();
    for (size_t i = 0; i < n_paths; ++i) {
        const swfr_path& p = paths[i];
        const bool wide = p.kind == SWFR_PATH_TOR && p.x_max - p.x_min > MAX_PATH_WIDTH;
        const int blocks = wide ? (p.x_max - p.x_min + MAX_PATH_WIDTH - 1) / MAX_PATH_WIDTH : 1;
        for (int k = 0; k < blocks; ++k) {
            swfr_path q = p;
            if (wide) { q.x_min = p.x_min + k * MAX_PATH_WIDTH; q.x_max = std::min(p.x_max, q.x_min + MAX_PATH_WIDTH); }
            q.first_edge = uint32_t(out_e.size());
            for (uint32_t j = 0; j < p.n_edges; ++j) {
                swfr_edge e = edges[p.first_edge + j];
                e.reserved = int32_t(out_p.size());
                out_e.push_back(e);
            }
            out_p.push_back(q);
        }
    }
    return true;
}

// bytes of the scene's read-only part in an arena (raw arrays + layout prefixes + sources), each piece padded
size_t scene_arena_bytes(const SceneLayout& L, const SceneView& sv) {
    auto P = SceneArena::padded;
    const size_t n_edges = sv.n_edges, n_paths = sv.n_paths, n_styles = sv.n_styles;
    // (a scene of solid colours only: the styles' {kind, pixel} heads, no filter records)
    return P(n_edges * sizeof(swfr_edge)) + P(n_paths * sizeof(swfr_path)) + (L.shader_level == 0 ? P(n_styles * 8) : P(n_styles * sizeof(swfr_style)) + P(n_styles * sizeof(DevFilter))) +
           P(L.fparams.size() * sizeof(int32_t)) + P(L.gradients.size() * sizeof(DevGradient)) + 3 * P((n_paths + 1) * sizeof(uint32_t)) +
           P((L.n_bands + 2) * sizeof(uint32_t)) + P(L.band_span.size() * sizeof(uint32_t)) + (L.any_blend ? P(n_paths + 64) : 0);
}
// pushes that part and fills the descriptor's scene fields
void push_scene(SceneArena& A, const SceneLayout& L, const SceneView& sv, Frame2& f) {
    const auto [edges, n_edges, paths, n_paths, styles, n_styles] = sv;
    f.raw = static_cast<swfr_edge*>(A.push(edges, n_edges * sizeof(swfr_edge)));
    f.paths = static_cast<DevPath*>(A.push(paths, n_paths * sizeof(swfr_path)));
    static_assert(offsetof(swfr_style, kind) == 0 && offsetof(swfr_style, pixel) == 4, "the head of a style is {kind, pixel}");
    if (L.shader_level == 0) {
        // solid colours only: the kernels read a style's kind and pixel and nothing else, so only those eight bytes travel
        uint32_t* heads = reinterpret_cast<uint32_t*>(A.host + A.used);
        for (size_t i = 0; i < n_styles; ++i) { heads[2 * i] = styles[i].kind; heads[2 * i + 1] = styles[i].pixel; }
        f.styles = reinterpret_cast<const swfr_style*>(A.push(nullptr, n_styles * 8));
        f.style_stride = 8;
        f.src.filters = nullptr;
    } else {
        f.styles = static_cast<swfr_style*>(A.push(styles, n_styles * sizeof(swfr_style)));
        f.style_stride = uint32_t(sizeof(swfr_style));
        f.src.filters = static_cast<DevFilter*>(A.push(L.filters.data(), n_styles * sizeof(DevFilter)));
    }
    f.src.fparams = static_cast<int32_t*>(A.push(L.fparams.data(), L.fparams.size() * sizeof(int32_t)));
    f.src.gradients = static_cast<DevGradient*>(A.push(L.gradients.data(), L.gradients.size() * sizeof(DevGradient)));
    f.n_linear_records = L.n_linear ? uint32_t(L.gradients.size()) : 0u; f.pad_linear = 0;
    f.path_chunks = static_cast<uint32_t*>(A.push(L.chunk_base.data(), (n_paths + 1) * sizeof(uint32_t)));
    f.path_slots = static_cast<uint32_t*>(A.push(L.slot_base.data(), (n_paths + 1) * sizeof(uint32_t)));
    f.path_inc = static_cast<uint32_t*>(A.push(L.inc_base.data(), (n_paths + 1) * sizeof(uint32_t)));
    f.band_off = static_cast<uint32_t*>(A.push(L.band_off.data(), (L.n_bands + 2) * sizeof(uint32_t)));
    f.path_bands = static_cast<uint32_t*>(A.push(L.band_span.data(), L.band_span.size() * sizeof(uint32_t)));
    f.path_op = nullptr;
    if (L.any_blend) {
        // the ABI's blend field split: the device's path record keeps lerp & 1 (0 for a blended path: no kernel may take one for a lerp
        // or a cover), the operator byte goes to a table of its own that only k2_tiles<3> and <4> read
        swfr_path* staged_paths = reinterpret_cast<swfr_path*>(A.host + (reinterpret_cast<const uint8_t*>(f.paths) - A.dev));
        uint8_t* ops = A.host + A.used;
        for (size_t i = 0; i < n_paths; ++i) { ops[i] = uint8_t(staged_paths[i].lerp >> 8); staged_paths[i].lerp &= 1u; }
        std::memset(ops + n_paths, 0, 64);
        f.path_op = static_cast<const uint8_t*>(A.push(nullptr, n_paths + 64));
    }
}
void fill_frame_sizes(const swfr_renderer* r, const SceneLayout& L, const SceneView& sv, Frame2& f) {
    f.n_edges = uint32_t(sv.n_edges); f.n_paths = uint32_t(sv.n_paths); f.n_chunks = uint32_t(L.n_chunks);
    f.n_bands = uint32_t(L.n_bands); f.n_strips = uint32_t(L.n_strips); f.n_strip_slots = uint32_t(L.n_strip_slots); f.cell_slice = uint32_t(L.cell_total); f.slow_cap = uint32_t(L.n_rows + 64);
    f.width = int32_t(r->width); f.height = int32_t(r->height); f.tiles_x = int32_t((r->width + TILE_W - 1) / TILE_W);
    f.fast_limit = uint32_t(std::min(std::max(r->fast_limit, 0), 16));       // (the row kernel's instance caps it at its own slots: 8 or 16)
    const BandShare bs = band_share(r);
    f.band_first = bs.first; f.band_stride = bs.stride;
    f.cell_main = uint32_t(L.cell_main);
    f.chunk_rows = L.chunk_rows; f.chunk_cap = uint32_t(L.n_chunks + 1); f.strip_order = r->strip_order ? 1u : 0u;
    f.mono = r->mono ? 1u : 0u;
}

// ---- colour-transformed textures ("Colour transforms")
constexpr size_t CX_TABLE_BYTES = 256 * sizeof(uint32_t);
// Waits for every stream of the handle once per call before the first texture of the cache is freed or reused: a texture outside the
// call and outside the resident scene can only be read by frames that were queued before the call.
void cx_quiesce(swfr_renderer* r) {
    if (r->cx_synced_epoch == r->cx_epoch) return;
    for (auto& x : r->fs) if (x.stream) HIP_CHECK(hipStreamSynchronize(x.stream));
    for (auto& g : r->groups) if (g.stream) HIP_CHECK(hipStreamSynchronize(g.stream));
    r->cx_synced_epoch = r->cx_epoch;
}
bool cx_stale(const swfr_renderer* r, const CxVariant& v) {
    const auto it = r->bitmaps.find(v.bitmap);
    return it == r->bitmaps.end() || it->second.gen != v.gen;
}
// The bitmap's straight texels on the device, ordered before whatever is queued on `st` next.  The first use uploads them on `st` (a
// hipMemcpy from pageable memory may return before its DMA has landed, and the frame streams are not ordered behind the null stream)
// and records an event behind the copy; a later use on another stream -- the next frame set of swfr_render_batch, the other batch group
// -- waits for that event on the device until it is known to have completed.  bm.straight stays until the bitmap is registered again.
void cx_straight_on(DeviceBitmap& bm, hipStream_t st) {
    if (!bm.d_straight) {
        const size_t bytes = size_t(bm.width) * bm.height * 4;
        if (!bm.straight_ready) HIP_CHECK(hipEventCreateWithFlags(&bm.straight_ready, hipEventDisableTiming));
        uint8_t* d = nullptr;
        HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&d), bytes));
        try {
            HIP_CHECK(hipMemcpyAsync(d, bm.straight.data(), bytes, hipMemcpyHostToDevice, st));
            HIP_CHECK(hipEventRecord(bm.straight_ready, st));
        } catch (...) {                                           // (never left half uploaded: the next use uploads again)
            (void)hipFree(d);
            throw;
        }
        bm.d_straight = d;
        bm.straight_stream = st;
        bm.straight_done = false;
        return;
    }
    if (!bm.straight_done && bm.straight_stream != st) {
        if (hipEventQuery(bm.straight_ready) == hipSuccess) bm.straight_done = true;
        else HIP_CHECK(hipStreamWaitEvent(st, bm.straight_ready, 0));
    }
}
// Evicts textures (stale generations first, then the least recently used) until `bytes` more fit the budget or nothing else may go;
// a texture of exactly `bytes` is handed back for reuse (its buffer and event) instead of being freed.
CxVariant cx_make_room(swfr_renderer* r, size_t bytes) {
    CxVariant reuse;
    while (r->cx_bytes + bytes > r->cx_budget) {
        auto victim = r->cx_cache.end();
        bool victim_stale = false;
        for (auto it = r->cx_cache.begin(); it != r->cx_cache.end(); ++it) {
            const CxVariant& v = it->second;
            if (v.pinned || v.used_epoch == r->cx_epoch) continue;
            const bool st = cx_stale(r, v);
            if (victim == r->cx_cache.end() || (st && !victim_stale) || (st == victim_stale && v.last_use < victim->second.last_use)) {
                victim = it;
                victim_stale = st;
            }
        }
        if (victim == r->cx_cache.end()) break;                // the rest is in use: this call goes over the budget
        cx_quiesce(r);
        CxVariant& v = victim->second;
        if (!reuse.pixels && v.bytes == bytes) reuse = v;
        else {
            HIP_CHECK(hipFree(v.pixels));
            if (v.ready) HIP_CHECK(hipEventDestroy(v.ready));
        }
        r->cx_bytes -= v.bytes;
        r->cx_cache.erase(victim);
    }
    return reuse;
}
// The textures a scene's colour-transformed bitmap styles sample (swfr_style::bitmap = VARIANT_BASE + k, k into the builder's
// variants()): from the cache, or made by the texel pass queued on `st` ahead of the frame.  Fills r->variant_table for
// prepare_sources.  pin: the scene goes to the resident slot -- its textures stay until the next scene replaces it there.
void resolve_variants(swfr_renderer* r, const SceneView& sv, hipStream_t st, bool pin) {
    const auto [edges, n_edges, paths, n_paths, styles, n_styles] = sv;
    r->variant_table.clear();
    if (pin) {
        for (const std::string& key : r->cx_pins) {
            const auto it = r->cx_cache.find(key);
            if (it != r->cx_cache.end()) it->second.pinned = false;
        }
        r->cx_pins.clear();
    }
    bool any = false;
    for (size_t i = 0; i < n_styles && !any; ++i) any = styles[i].kind == SWFR_STYLE_BITMAP && styles[i].bitmap >= VARIANT_BASE && styles[i].bitmap < BLUR_BASE;
    if (!any) return;                                             // (a scene without colour-transformed bitmaps: nothing at all)
    const auto& V = r->builder->variants();
    r->variant_table.assign(V.size(), DevBitmap{nullptr, 0, 0});
    for (size_t i = 0; i < n_paths; ++i) {
        const swfr_style& s = styles[paths[i].style];
        if (s.kind != SWFR_STYLE_BITMAP || s.bitmap < VARIANT_BASE || s.bitmap >= BLUR_BASE) continue;
        const uint32_t k = s.bitmap - VARIANT_BASE;               // (validate_scene: k < V.size(), the bitmap is registered)
        if (r->variant_table[k].pixels) continue;
        const TextureVariant& tv = V[k];
        DeviceBitmap& bm = r->bitmaps.at(tv.bitmap);
        // (arrays built before the bitmap was captured or blurred: it has no straight texels for the texel pass any more)
        if (bm.captured) throw StatusError{SWFR_ERR_NOT_IMPLEMENTED, "NotImplementedCapturedBitmapTransform"};
        std::string key(sizeof(uint32_t) + sizeof(uint64_t) + sizeof(ColorLut), '\0');
        std::memcpy(&key[0], &tv.bitmap, sizeof(uint32_t));
        std::memcpy(&key[sizeof(uint32_t)], &bm.gen, sizeof(uint64_t));
        std::memcpy(&key[sizeof(uint32_t) + sizeof(uint64_t)], &tv.lut, sizeof(ColorLut));
        auto it = r->cx_cache.find(key);
        if (it == r->cx_cache.end()) {
            const size_t n = size_t(bm.width) * bm.height, bytes = n * 4;
            cx_straight_on(bm, st);
            CxVariant v = cx_make_room(r, bytes);
            if (!v.pixels) HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&v.pixels), bytes + CX_TABLE_BYTES));   // (the chain's table behind the texels)
            r->cx_bytes += bytes;
            v.bytes = bytes;
            it = r->cx_cache.emplace(key, v).first;
            CxVariant& e = it->second;
            try {
                if (!e.ready) HIP_CHECK(hipEventCreateWithFlags(&e.ready, hipEventDisableTiming));
                e.bitmap = tv.bitmap; e.gen = bm.gen; e.stream = st; e.done = false; e.pinned = false;
                e.table.reset(new uint32_t[256], std::default_delete<uint32_t[]>());
                for (int c = 0; c < 256; ++c)
                    e.table.get()[c] = uint32_t(tv.lut.t[0][c]) | uint32_t(tv.lut.t[1][c]) << 8 | uint32_t(tv.lut.t[2][c]) << 16 | uint32_t(tv.lut.t[3][c]) << 24;
                HIP_CHECK(hipMemcpyAsync(e.pixels + n, e.table.get(), CX_TABLE_BYTES, hipMemcpyHostToDevice, st));
                launch_cxform_texels(st, bm.d_straight, e.pixels, n, e.pixels + n);
                HIP_CHECK(hipGetLastError());
                HIP_CHECK(hipEventRecord(e.ready, st));
            } catch (...) {                                       // a texture that was not made never stays in the cache
                (void)hipFree(e.pixels);
                if (e.ready) (void)hipEventDestroy(e.ready);
                r->cx_bytes -= bytes;
                r->cx_cache.erase(it);
                throw;
            }
        } else {
            CxVariant& e = it->second;
            // made on another stream and maybe still running: this frame's stream waits for it on the device
            if (!e.done && e.stream != st) {
                if (hipEventQuery(e.ready) == hipSuccess) e.done = true;
                else HIP_CHECK(hipStreamWaitEvent(st, e.ready, 0));
            }
        }
        CxVariant& e = it->second;
        e.used_epoch = r->cx_epoch;
        e.last_use = ++r->cx_tick;
        if (pin && !e.pinned) { e.pinned = true; r->cx_pins.push_back(key); }
        r->variant_table[k] = DevBitmap{e.pixels, bm.width, bm.height};
    }
}

// The host preparation of a frame, one for every route: isolated groups lowered (frames with a group only), paths wider than 8192 px
// split into column blocks (frames that wide only), the colour-transformed textures resolved on the paths as drawn -- queued on `st`,
// pinned for the resident slot -- and the layout worked out into L.  A step that does not apply copies nothing: the arrays returned are
// the ones passed in, or live in S, which has to outlive their use.  The edges carry their path index in `reserved`.
struct FrameScratch { std::vector<swfr_edge> group_e, split_e; std::vector<swfr_path> group_p, split_p; std::vector<swfr_style> group_s; };
SceneView prepare_frame(swfr_renderer* r, SceneView a, hipStream_t st, bool pin, FrameScratch& S, SceneLayout& L) {
    bool faded = false;
    if (lower_groups(a, S.group_e, S.group_p, S.group_s, faded))
        a = SceneView{S.group_e.data(), S.group_e.size(), S.group_p.data(), S.group_p.size(), S.group_s.data(), S.group_s.size()};
    const SceneView drawn = a;                                        // the paths as drawn: a style is anchored at their rectangles
    const bool split = split_wide_paths(a, S.split_e, S.split_p);
    if (split) { a.edges = S.split_e.data(); a.n_edges = S.split_e.size(); a.paths = S.split_p.data(); a.n_paths = S.split_p.size(); }
    resolve_variants(r, drawn, st, pin);
    layout_scene(r, a, L, split ? &drawn : nullptr, faded);
    return a;
}

// The bounds part of a launch plan -- what the grids of the kernels are sized by -- of one laid-out frame: every other field is zero
LaunchPlan plan_bounds(const SceneLayout& L, size_t n_edges, size_t n_paths) {
    LaunchPlan p{};
    p.max_edges = uint32_t(n_edges); p.max_paths = uint32_t(n_paths); p.max_bands = uint32_t(L.n_bands);
    p.max_chunks = uint32_t(L.n_chunks); p.max_path_edges = L.max_path_edges; p.rows_wide = L.rows_wide;
    p.linear_grid = L.n_linear ? uint32_t(L.gradients.size()) : 0u;
    p.max_strips = uint32_t(L.n_strip_slots); p.shader_level = L.shader_level;
    return p;
}
// ... of several frames in one launch: the maxima of theirs (the wide row kernel when one of them asks for it)
void merge_bounds(LaunchPlan& p, const LaunchPlan& q) {
    p.max_edges = std::max(p.max_edges, q.max_edges); p.max_paths = std::max(p.max_paths, q.max_paths); p.max_bands = std::max(p.max_bands, q.max_bands);
    p.max_chunks = std::max(p.max_chunks, q.max_chunks); p.max_path_edges = std::max(p.max_path_edges, q.max_path_edges); p.rows_wide = p.rows_wide || q.rows_wide;
    p.linear_grid = std::max(p.linear_grid, q.linear_grid); p.max_strips = std::max(p.max_strips, q.max_strips); p.shader_level = std::max(p.shader_level, q.shader_level);
}
// Points a frame's descriptor at its share of a work and a cls allocation (frame_layout.hpp) and moves w and c on to the next frame's;
// ahead: f is the frame's parity-1 descriptor (a copy of the parity-0 one), which gets buffers of its own for what k2_bin writes
void place_frame(Frame2& f, const FrameDims& d, size_t tiles_x, uint8_t*& w, uint8_t*& c, bool ahead = false) {
    w = ahead ? carve_frame_ahead(f, d, w) : carve_frame(f, d, w);
    set_cls_region(f, d, tiles_x, c);
    c += pad256(cls_region_bytes(d, tiles_x));
}

// Uploads a scene -- the raw edge list, the paths and the styles, plus the layout above -- and sizes the buffers the
// kernels write.
int upload2(swfr_renderer* r, int si, bool all_sets, SceneView sv, uint32_t* fb_override, bool edges_tagged) {
    swfr_renderer::Scene& sc = r->scn[si];
    if (si == 0) r->scene_ready = false;
    if (r->async_used) {
        // frames queued by swfr_render_resident_async may still read the scene and the buffers this call rewrites
        for (int k = 0; k < 4; ++k) if (r->fs[k].stream) HIP_CHECK(hipStreamSynchronize(r->fs[k].stream));
    }
    // which of the queued-row kernels the frame needs: assumed to be what the previous frame needed (an animation's frames are
    // alike), checked against the frame's own counters afterwards (render_resident renders again with everything if not)
    sc.slow_verified = false;
    sc.slow_state = si == 0 ? r->hint_slow_state : 0; sc.slow_passes = si == 0 ? r->hint_slow_passes : SLOW_PASSES;
    if (si > 0 && !r->fs[si].stream) HIP_CHECK(hipStreamCreateWithFlags(&r->fs[si].stream, hipStreamNonBlocking));
    const hipStream_t up_stream = r->fs[si].stream;
    const uint32_t tiles_x = (r->width + TILE_W - 1) / TILE_W;
    std::vector<swfr_edge> tagged;
    if (!edges_tagged) {
        tagged.assign(sv.edges, sv.edges + sv.n_edges);
        for (size_t i = 0; i < sv.n_paths; ++i)
            for (uint32_t k = 0; k < sv.paths[i].n_edges; ++k) tagged[sv.paths[i].first_edge + k].reserved = int32_t(i);
        // an aliased handle paints a caller's boxes as the frame builder makes them: rounded to whole pixels (a box that rounds away covers nothing)
        if (r->mono)
            for (size_t i = 0; i < sv.n_paths; ++i)
                if (sv.paths[i].kind == SWFR_PATH_BOXES)
                    for (uint32_t k = 0; k < sv.paths[i].n_edges; ++k) round_box_to_pixels(tagged[sv.paths[i].first_edge + k]);
        sv.edges = tagged.data();
    }
    static thread_local FrameScratch scratch;              // (vectors keep their capacity from frame to frame)
    static thread_local SceneLayout L;
    const SceneView a = prepare_frame(r, sv, up_stream, si == 0, scratch, L);
    const FrameDims dims = sc.dims = FrameDims::of_layout(L, a.n_edges, a.n_paths);
    sc.bounds = plan_bounds(L, a.n_edges, a.n_paths);
    SceneArena& A = sc.arena;
    A.begin(scene_arena_bytes(L, a) + SceneArena::padded(8 * sizeof(Frame2)) + 4096);
    Frame2 proto;
    std::memset(&proto, 0, sizeof proto);
    push_scene(A, L, a, proto);
    fill_frame_sizes(r, L, a, proto);
    if (r->bitmap_table_dirty) r->d_bitmap_table.reserve(r->bitmap_table.size());     // (filled below; the address is what the descriptor needs)
    proto.src.bitmaps = r->d_bitmap_table.ptr;
    sc.proto = proto;
    // ---- per-frame (kernel-written) buffers: two grow-only allocations per frame set, carved by the list in frame_layout.hpp, and the sets' descriptors
    const size_t cls_bytes = cls_region_bytes(dims, tiles_x);
    const int n_sets = int(sets_wanted(r));
    // A scene uploaded into every frame set (swfr_upload_edges, or several resident frames of the builder's scene) gets two descriptors
    // per set, parity 0 and 1: a copy each of what k2_bin writes or clears, the rest shared, so that render_resident can bin a set's next
    // frame beside the row pass of the one before.  Every other route launches with parity 0, which lies where it always did.
    const bool ahead = all_sets && r->bin_ahead && !r->mono && r->cfg.band_count <= 1;
    Frame2 fr[8];                                                     // [0, 4): the sets' parity-0 descriptors, [4, 8): their parity-1 ones
    std::memset(fr, 0, sizeof fr);
    for (int k = 0; k < 4; ++k) {
        if (all_sets ? k >= n_sets : k != si) continue;
        auto& x = r->fs[k];
        Frame2& f = fr[k];
        f = proto;
        if (!x.stream) HIP_CHECK(hipStreamCreateWithFlags(&x.stream, hipStreamNonBlocking));
        x.work.reserve(frame_work_bytes(dims) + (ahead ? frame_ahead_bytes(dims) : 0)); x.cls.reserve(ahead ? pad256(cls_bytes) + cls_bytes : cls_bytes);
        uint8_t *w = x.work.ptr, *c = x.cls.ptr;
        place_frame(f, dims, tiles_x, w, c);
        // two buffers keep places of their own instead of the carved ones.  The strip costs: the next scene's sizes would move them, and
        // the costs one frame leaves order the strips of the next whatever scene that is (zero between frames: the ordering workgroup
        // clears what it has read; cleared here on fresh memory only).  The counters: one copy brings all sets' back
        const uint32_t* cost_before = x.strip_cost.ptr;
        x.strip_cost.reserve(dims.strip_cost_count());
        if (x.strip_cost.ptr != cost_before) HIP_CHECK(hipMemsetAsync(x.strip_cost.ptr, 0, x.strip_cost.cap * sizeof(uint32_t), up_stream));
        f.strip_cost = x.strip_cost.ptr;
        r->d_counters.reserve(8 * COUNTER_WORDS);
        f.counters = x.counters = r->d_counters.ptr + size_t(k) * COUNTER_WORDS;
        // class bytes outside the paths' rectangles are never written by a kernel: cleared once per uploaded scene (both parities' at once)
        HIP_CHECK(hipMemsetAsync(x.cls.ptr, 0, ahead ? pad256(cls_bytes) + cls_bytes : cls_bytes, up_stream));
        if (!x.d_fb.ptr && !r->n_targets) {                                             // (a handle with caller targets never renders into a buffer of its own)
            x.d_fb.reserve(size_t(r->width) * r->height);
            HIP_CHECK(hipMemsetAsync(x.d_fb.ptr, 0, size_t(r->width) * r->height * 4, up_stream));
        }
        f.fb = (fb_override && k == si) ? fb_override : (r->n_targets ? r->targets[uint32_t(k) % r->n_targets] : x.d_fb.ptr);
        if (ahead) {
            Frame2& f1 = fr[4 + k];
            f1 = f;                                                                      // (the shared buffers, the framebuffer)
            place_frame(f1, dims, tiles_x, w, c, true);
            const uint32_t* cost1_before = x.strip_cost_ahead.ptr;
            x.strip_cost_ahead.reserve(dims.strip_cost_count());
            if (x.strip_cost_ahead.ptr != cost1_before) HIP_CHECK(hipMemsetAsync(x.strip_cost_ahead.ptr, 0, x.strip_cost_ahead.cap * sizeof(uint32_t), up_stream));
            f1.strip_cost = x.strip_cost_ahead.ptr;
            f1.counters = r->d_counters.ptr + size_t(4 + k) * COUNTER_WORDS;
        }
    }
    sc.frames_dev = static_cast<Frame2*>(A.push(fr, sizeof fr));
    sc.frames_ahead = ahead ? sc.frames_dev + 4 : nullptr;
    A.flush(up_stream, si == 0);
    if (all_sets) {
        // the copy and the memsets above ran on set `si`'s stream: the other sets' streams start their frames behind them
        for (int k = 0; k < n_sets; ++k)
            if (k != si && r->fs[k].stream) HIP_CHECK(hipStreamWaitEvent(r->fs[k].stream, A.copied, 0));
    }
    if (r->bitmap_table_dirty) {
        if (!r->bitmap_table.empty())
            HIP_CHECK(hipMemcpyAsync(r->d_bitmap_table.ptr, r->bitmap_table.data(), r->bitmap_table.size() * sizeof(DevBitmap),
                                     hipMemcpyHostToDevice, r->stream));
        r->bitmap_table_dirty = false;
        r->bitmap_table_dirty_copied = true;
    }
    if (r->bitmap_table_dirty_copied) { HIP_CHECK(hipStreamSynchronize(r->stream)); r->bitmap_table_dirty_copied = false; }   // bitmap_table may be edited next
    if (si == 0) { r->scene_ready = true; r->sets_ready = all_sets ? uint32_t(n_sets) : 1u; r->scene_from_builder = edges_tagged; ++r->scene_gen; }
    return SWFR_OK;
}

// A scene with a SWFR_STYLE_LINEAR_PIXMAN style: everything such a style is refused for, by a host-only handle too -- an unknown kind
// beside it, an aliased handle, c0 == c1, and what prepare_sources / linear_of find (pieces, range, row step), by a dry run of theirs.
void validate_linear_pixman(const swfr_renderer* r, const SceneView& sv) {
    const auto [edges, n_edges, paths, n_paths, styles, n_styles] = sv;
    bool any = false;
    for (size_t i = 0; i < n_styles; ++i) any = any || styles[i].kind >= SWFR_STYLE_LINEAR_PIXMAN;
    if (!any) return;
    for (size_t i = 0; i < n_styles; ++i) {
        const swfr_style& s = styles[i];
        if (s.kind > SWFR_STYLE_LINEAR_PIXMAN) throw StatusError{SWFR_ERR_INVALID, "unknown style kind"};
        if (s.kind != SWFR_STYLE_LINEAR_PIXMAN) continue;
        if (r->mono) throw StatusError{SWFR_ERR_NOT_IMPLEMENTED, "NotImplementedAliasedPixmanLinear"};
        if (s.n_stops > SWFR_MAX_STOPS) throw StatusError{SWFR_ERR_INVALID, "too many gradient stops"};
        if (s.c0x == s.c1x && s.c0y == s.c1y) throw StatusError{SWFR_ERR_INVALID, "a pixman-linear gradient needs two distinct points (c0 == c1)"};
        // only the line of a SWF fill, (-16384, 0)-(16384, 0), has been held against libcairo (with it Cairo's fit-to-range scaling
        // always applies); any other line is refused, not trusted
        if (s.c0x != -16384.0 || s.c0y != 0.0 || s.c1x != 16384.0 || s.c1y != 0.0) throw StatusError{SWFR_ERR_NOT_IMPLEMENTED, "NotImplementedLinearLine"};
    }
    for (size_t i = 0; i < n_paths; ++i) {                            // (a malformed path is validate_scene's to name)
        const swfr_path& p = paths[i];
        if (size_t(p.first_edge) + p.n_edges > n_edges || (p.kind < SWFR_PATH_GROUP_BEGIN && p.style >= n_styles) || p.kind > SWFR_PATH_GROUP_MASK) return;
        if (p.x_min < 0 || p.y_min < 0 || p.x_max > int(r->width) || p.y_max > int(r->height) || p.x_min > p.x_max || p.y_min > p.y_max) return;
    }
    std::vector<DevFilter> filters; std::vector<DevGradient> gradients; std::vector<int32_t> fparams; size_t n_linear = 0;
    std::vector<swfr_style> only;                                     // (the other kinds need tables a host-only handle may not have)
    only.assign(styles, styles + n_styles);
    for (swfr_style& s : only) if (s.kind != SWFR_STYLE_LINEAR_PIXMAN) { s.kind = SWFR_STYLE_SOLID; }
    std::vector<swfr_path> drawn;                                     // (a group marker has no style of its own before lower_groups)
    for (size_t i = 0; i < n_paths; ++i) if (paths[i].kind < SWFR_PATH_GROUP_BEGIN) drawn.push_back(paths[i]);
    prepare_sources(SceneView{edges, n_edges, drawn.data(), drawn.size(), only.data(), n_styles}, false, n_linear, filters, gradients, fparams, r->bitmap_table, r->variant_table, r->blur_table);
}

// Everything a caller-supplied scene is refused for before it is uploaded (swfr_upload_edges).  The order is behaviour: it decides which
// refusal a scene with several faults gets, and what a host-only handle still names before it refuses to rasterize
void validate_upload(const swfr_renderer* r, const SceneView& sv) {
    const bool alpha_modes = (r->cfg.flags & SWFR_FLAG_ALPHA_MODES) != 0;
    validate_groups(sv, alpha_modes);
    validate_blend_fields(sv, alpha_modes);                      // (a malformed blend field is refused as such even by a host-only handle)
    validate_gradient_extend(sv);                                // (and so is a gradient's extend)
    validate_bitmap_filter(sv);                                  // (and a bitmap's filter)
    validate_linear_pixman(r, sv);                               // (and what a pixman-linear style cannot be drawn with)
    if (!r->has_device) throw StatusError{SWFR_ERR_NO_DEVICE, "host-only handle cannot rasterize"};
    validate_scene(r, sv);
}

// The frames of one launch chain: `n` descriptors from `cur` on (blockIdx.y = frame).  binned: an earlier row launch has run their k2_bin,
// the chain starts at the row pass.  next: the row launch also bins these `n_next` frames, the same frame sets' other parity
// (k2_rows_ahead_b) -- only under a plan that bins_ahead() admits.
struct ChainFrames { const Frame2* cur; uint32_t n; bool binned = false; const Frame2* next = nullptr; uint32_t n_next = 0; };

// THE launch chain: bin -> rows -> queued rows -> linear pieces -> tiles, or in its fused form (bin ->) rows + the next frames' bin ->
// tiles.  events (optional): four, recorded around the three passes.
// fb_to: the one frame's own target instead of its descriptor's (swfr_render_resident_async_to), else nullptr.
void launch_chain(swfr_renderer* r, hipStream_t st, const ChainFrames& f, const LaunchPlan& p, hipEvent_t* events, uint32_t* fb_to) {
    if (events) HIP_CHECK(hipEventRecord(events[0], st));
    if (!f.binned) {
        r->last_bin_threads = p.bin_threads;
        launch2_bin(st, f.cur, f.n, p.max_edges, p.max_paths, p.max_bands, p.slow_kernels, r->mono, p.bin_threads);
    }
    if (events) HIP_CHECK(hipEventRecord(events[1], st));
    if (f.next) {
        launch2_rows_ahead(st, f.cur, f.next, f.n, f.n_next, p.max_edges, p.max_paths, p.max_bands, p.max_chunks);
        ++r->last_ahead_launches;
    } else {
        launch2_rows(st, f.cur, f.n, p.max_chunks, p.max_path_edges, p.rows_wide, r->mono);
        if (p.run_slow) launch2_rows_slow(st, f.cur, f.n, p.grid_slow, p.grid_huge, p.slow_passes, r->mono);
        launch2_linear_pieces(st, f.cur, f.n, p.linear_grid);      // (pixman-linear tor paths: where libcairo starts each row's ramps; timed with the row pass)
    }
    if (events) HIP_CHECK(hipEventRecord(events[2], st));
    launch2_tiles(st, f.cur, f.n, p.max_strips, p.tiles_grid, p.shader_level, fb_to);
    if (events) HIP_CHECK(hipEventRecord(events[3], st));
}
// k2_bin's instance for a launch whose frames have up to max_paths paths: SWFR_BIN_THREADS when set, else the small one where no frame
// needs a second round of its tile-row step and other frames run beside the launch (`overlapped`, as in launch_frame): its
// four-wavefront workgroups start in the slots the other frames' row and tile passes free one at a time, where a sixteen-wavefront
// workgroup waits for half a CU ("k2_bin sized to the scene").  A frame that has the GPU to itself keeps the
// large instance: its ordering workgroups have four times the threads for the same strips.
uint32_t bin_threads_of(const swfr_renderer* r, uint32_t max_paths, bool overlapped) {
    if (r->bin_threads) return uint32_t(r->bin_threads);
    return overlapped && max_paths <= BIN_SMALL_PATHS ? BIN_THREADS_SMALL : BIN_THREADS_LARGE;
}
// The plan of the resident scene's frames, as a frame launched on its own frame set gets it; the routes that differ say so where they call.
LaunchPlan plan_of(const swfr_renderer* r, const swfr_renderer::Scene& sc) {
    LaunchPlan p = sc.bounds;
    p.run_slow = p.max_chunks && sc.slow_state != 1;           // the queued rows: skipped once a frame of this resident scene has shown there are none
    p.slow_kernels = p.run_slow ? 1u : 0u;
    p.bin_threads = bin_threads_of(r, p.max_paths, true);
    p.grid_slow = 1024u; p.grid_huge = sc.slow_state == 2 ? 0u : 256u; p.slow_passes = sc.slow_passes;
    p.tiles_grid = r->tiles_grid > 0 ? uint32_t(r->tiles_grid) : ~0u;
    return p;
}

// the kernels of one frame of scene `sc` on frame set `F`, writing the framebuffer `fb`; e (optional): four events around them
// overlapped: other frames run beside this one (several frame sets in flight) -- the tile pass is then launched in its paired shape (two
// strips per wavefront, better for the frame rate); a frame that has the GPU to itself (a blocking swfr_render, a handle with one frame
// in flight) gets one wavefront per strip, which finishes 2-3 us sooner ("Two strips per wavefront")
void launch_frame(swfr_renderer* r, const swfr_renderer::Scene& sc, swfr_renderer::FrameSet& F, uint32_t* fb, hipEvent_t* e, bool overlapped) {
    LaunchPlan plan = plan_of(r, sc);
    if (r->tiles_grid <= 0 && !overlapped) plan.tiles_grid = 0x7fffffffu;      // (a frame alone: one wavefront per strip)
    plan.bin_threads = bin_threads_of(r, plan.max_paths, overlapped);
    // the frame's descriptor (scene arrays, this set's buffers, the framebuffer) was uploaded with the scene
    launch_chain(r, F.stream, {sc.frames_dev + (&F - r->fs), 1}, plan, e, fb);   // (fb: this frame's own target, else the descriptor's)
}

int check_counters(swfr_renderer* r, const uint32_t* counters) {
    const uint32_t err = counters[C2_ERROR];
    r->stats.frames += 1; r->stats.queued_rows += counters[C2_SLOW]; r->stats.crowded_rows += counters[C2_HUGE];
    r->stats.tie_rows += counters[C2_TIE_ROWS];
    r->stats.pairtest_limit += counters[C2_TIE_PAIRTEST_SKIPPED] ? 1 : 0;
    r->stats.start_group_limit += ((err & (E2_ACTIVE_EDGES | E2_START_GROUP)) || counters[C2_TIE_SORT_OVERFLOW]) ? 1 : 0;
    r->stats.history_limit += counters[C2_TIE_DEPTH] ? 1 : 0;
    if (err & ~(E2_ACTIVE_EDGES | E2_START_GROUP | E2_CELL_ARENA)) {
        r->fb_valid = false;
        return fail(r, SWFR_ERR_DEVICE, "internal consistency check failed in the raster kernels (code " + std::to_string(err) + ")");
    }
    if (err) {
        r->fb_valid = false;
        return fail(r, SWFR_ERR_CAPACITY, err & E2_CELL_ARENA ? "cell arena exhausted (uneven allocator shares)" :
                    "a pixel row has more than 8192 active edges of one path, or more than 8192 of its edges start at one sample row (scan converter capacity)");
    }
    // the replay of Cairo's edge-list order for coincident edges has capacity limits; a scene that reaches one is refused,
    // never rendered approximately
    if (counters[C2_TIE_PAIRTEST_SKIPPED] | counters[C2_TIE_SORT_OVERFLOW] | counters[C2_TIE_DEPTH]) {
        r->fb_valid = false;
        return fail(r, SWFR_ERR_CAPACITY, std::string("coincident edges beyond the capacity of the list-order replay (") +
                    (counters[C2_TIE_PAIRTEST_SKIPPED] ? "crossing test over more than 2^21 edge pairs; " : "") +
                    (counters[C2_TIE_SORT_OVERFLOW] ? "more than 16 edges starting at one sample row; " : "") +
                    (counters[C2_TIE_DEPTH] ? "tie history deeper than two levels; " : "") + ")");
    }
    return SWFR_OK;
}
// The read-back of frames' counters, in two halves with the wait for `st` between them.  queue_counters: the copy of n frames'
// counters to (pinned) host memory, queued on the frames' stream behind their kernels -- n contiguous ones from `dev` on in one
// copy, or one copy each for the n descriptors of a launch.
void queue_counters(hipStream_t st, uint32_t* host, const uint32_t* dev, uint32_t n = 1) {
    HIP_CHECK(hipMemcpyAsync(host, dev, size_t(n) * COUNTER_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
}
void queue_counters(hipStream_t st, uint32_t* host, const Frame2* fr, uint32_t n) {
    for (uint32_t k = 0; k < n; ++k) queue_counters(st, host + size_t(k) * COUNTER_WORDS, fr[k].counters);
}
// check_frames: check_counters over the n frames in order (swfr_stats accumulates in it), stopping at the first failure; rc: an earlier
// failure, which stands with nothing more checked.  launched_for: the frames ran with only the queued-row kernels that scene is known
// to need -- a frame that queued rows for the others is not valid, and is refused before its counters are checked.
int check_frames(swfr_renderer* r, const uint32_t* host, uint32_t n, int rc = SWFR_OK, const swfr_renderer::Scene* launched_for = nullptr) {
    for (uint32_t k = 0; k < n && rc == SWFR_OK; ++k) {
        const uint32_t* c = host + size_t(k) * COUNTER_WORDS;
        if (launched_for && ((launched_for->slow_state == 1 && c[C2_SLOW]) || (launched_for->slow_state == 2 && c[C2_HUGE])))
            rc = fail(r, SWFR_ERR_DEVICE, "queued rows without their kernels in a batched launch");
        if (rc == SWFR_OK) rc = check_counters(r, c);
    }
    return rc;
}
// the handle's pinned copy of d_counters: eight frames' worth
uint32_t* pinned_counters(swfr_renderer* r) {
    if (!r->h_counters) HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&r->h_counters), 8 * COUNTER_WORDS * sizeof(uint32_t), hipHostMallocDefault));
    return r->h_counters;
}

// One frame of the resident scene on frame set F as a graph launch: the set's kernels (with the queued-row kernels the scene is
// known to need) are captured from the set's own stream the first time and replayed afterwards; a new upload, or a change in what
// the scene needs of the queued-row kernels, captures again.
void ensure_frame_graph(swfr_renderer* r, const swfr_renderer::Scene& sc, swfr_renderer::FrameSet& F) {
    const uint64_t key = (r->scene_gen << 16) | (uint64_t(sc.slow_state & 3) << 8) | uint64_t(sc.slow_passes & 0xffu) | (uint64_t(1) << 63);
    if (F.graph_key != key) {
        if (F.graph_exec) { (void)hipGraphExecDestroy(F.graph_exec); F.graph_exec = nullptr; }
        if (F.graph) { (void)hipGraphDestroy(F.graph); F.graph = nullptr; }
        F.graph_key = 0;
        HIP_CHECK(hipStreamBeginCapture(F.stream, hipStreamCaptureModeRelaxed));
        try {
            launch_frame(r, sc, F, nullptr, nullptr, true);
        } catch (...) {
            hipGraph_t g = nullptr;
            (void)hipStreamEndCapture(F.stream, &g);
            if (g) (void)hipGraphDestroy(g);
            throw;
        }
        HIP_CHECK(hipStreamEndCapture(F.stream, &F.graph));
        HIP_CHECK(hipGraphInstantiate(&F.graph_exec, F.graph, nullptr, nullptr, 0));
        F.graph_key = key;
    }
}

// A mapped read-back that nobody has waited for yet (swfr_read_image_async) reads the last frame's framebuffer -- or its
// un-premultiplied copy -- on the handle's stream; frame sets 1..3 render on streams of their own and are not ordered behind it.
// Before anything is launched on them they wait for the copy ON THE DEVICE (no host wait; nothing at all when no read is pending),
// so that a frame can never be rasterized into the buffer the copy is still reading.
void order_frames_behind_pending_read(swfr_renderer* r) {
    if (!r->read_pending || !r->read_done) return;
    for (int k = 1; k < 4; ++k)
        if (r->fs[k].stream) HIP_CHECK(hipStreamWaitEvent(r->fs[k].stream, r->read_done, 0));
}

// ---- blurred layers ("Blurred layers")
// the routes that do not draw a blurred layer refuse the frame by name (swfr.h, SWFR_OBJECT_BLURRED_LAYER): never drawn unblurred
void refuse_blur_route(const swfr_renderer* r) {
    if (!r->builder->layers().empty()) throw StatusError{SWFR_ERR_NOT_IMPLEMENTED, "NotImplementedBlurRoute"};
}
// everything queued on any stream of the handle has finished: what swfr_capture_bitmap and swfr_blur_bitmap are ordered behind
void wait_all_streams(swfr_renderer* r) {
    for (auto& x : r->fs) if (x.stream) HIP_CHECK(hipStreamSynchronize(x.stream));
    for (auto& g : r->groups) if (g.stream) HIP_CHECK(hipStreamSynchronize(g.stream));
}
// The blur (blur_x, blur_y, passes) of the width x height image at `a`, the passes alternating between `a` and `b`, queued on `st`:
// returns where the result lies -- `a` after an even number of steps (blur_steps), `b` after an odd one.  swfr_shadow_bitmap's box
// passes only: every other route plans its passes (filter_plan.hpp) and runs them through run_filter_plan
uint32_t* blur_image(hipStream_t st, uint32_t* a, uint32_t* b, uint32_t width, uint32_t height, uint32_t blur_x, uint32_t blur_y, uint32_t passes) {
    for (uint32_t p = 0; p < passes; ++p)
        for (int vertical = 0; vertical < 2; ++vertical) {
            const uint32_t w = vertical ? blur_y : blur_x;
            if (w <= 1u) continue;
            launch_blur_pass(st, a, b, width, height, w, vertical != 0);
            std::swap(a, b);
        }
    HIP_CHECK(hipGetLastError());
    return a;
}
// Queues a plan's steps (filter_plan.hpp) on `st`, in order: the one place that maps a step to a launch.  bufs: the width x height
// buffers the plan names, indexed by Buffer (those it does not use may be null); list, kernels: the entries the plan was made of and,
// per convolution entry, its kernel
void run_filter_plan(hipStream_t st, const FilterPlan& plan, const swfr_filter* list, const swfr_kernel* kernels, uint32_t* const bufs[4], uint32_t width, uint32_t height) {
    const size_t n = size_t(width) * height;
    for (uint32_t k = 0; k < plan.n; ++k) {
        const FilterStep& s = plan.steps[k];
        const swfr_shadow& S = list[s.entry].shadow;
        const uint32_t* const src = bufs[s.src];
        uint32_t* const dst = bufs[s.dst];
        switch (s.op) {
        case Op::CAPTURE: launch_blur_capture(st, src, dst, n); break;
        case Op::BOX_H: launch_blur_pass(st, src, dst, width, height, S.blur_x, false); break;
        case Op::BOX_V: launch_blur_pass(st, src, dst, width, height, S.blur_y, true); break;
        case Op::SHADOW_ALPHA: launch_shadow_alpha(st, src, dst, width, height, S.dx, S.dy, (S.flags & SWFR_SHADOW_INNER) != 0u); break;
        case Op::SHADOW_FINISH: launch_shadow_finish(st, src, bufs[s.group], s.group == FB, dst, n, shadow_color_pixel(S.color), S.strength, S.flags); break;
        case Op::CONVOLVE: launch_convolve(st, src, dst, width, height, kernels[s.entry], s.src == FB); break;
        case Op::COPY: HIP_CHECK(hipMemcpyAsync(dst, src, n * 4, hipMemcpyDeviceToDevice, st)); break;
        }
    }
    HIP_CHECK(hipGetLastError());
}
// drops what a bitmap slot holds before it gets new texels: its device memory, and the colour-transformed textures made from it
void release_bitmap_slot(swfr_renderer* r, uint32_t id, DeviceBitmap& slot) {
    if (slot.pixels) HIP_CHECK(hipFree(slot.pixels));
    if (slot.d_straight) HIP_CHECK(hipFree(slot.d_straight));
    if (slot.straight_ready) HIP_CHECK(hipEventDestroy(slot.straight_ready));
    slot = DeviceBitmap{};
    for (auto it = r->cx_cache.begin(); it != r->cx_cache.end();) {
        if (it->second.bitmap == id && !it->second.pinned) {
            cx_quiesce(r);
            (void)hipFree(it->second.pixels);
            if (it->second.ready) (void)hipEventDestroy(it->second.ready);
            r->cx_bytes -= it->second.bytes;
            it = r->cx_cache.erase(it);
        } else ++it;
    }
}
// Slot `id` holds the w x h texels at `pixels`, made on the device (the slot's own, written in place, or a fresh allocation the slot
// takes over): a new generation -- stale colour-transformed variants go --, no straight texels.  in_place: a registered bitmap keeps
// its texture and size, and the builder only learns that it is captured; otherwise it is registered (again) and the table follows
void bitmap_slot_has_new_texels(swfr_renderer* r, uint32_t id, uint32_t* pixels, uint32_t w, uint32_t h, bool in_place) {
    DeviceBitmap& bm = r->bitmaps[id];
    if (bm.pixels == pixels) bm.pixels = nullptr;                // (kept: release_bitmap_slot frees what the slot holds)
    release_bitmap_slot(r, id, bm);
    bm.pixels = pixels; bm.width = w; bm.height = h;
    bm.gen = ++r->bitmap_gen;
    bm.captured = true;
    if (in_place) { r->builder->set_bitmap_captured(id); return; }
    BitmapInfo info{w, h};
    info.captured = true;
    r->builder->add_bitmap(id, info);
    if (r->bitmap_table.size() <= id) r->bitmap_table.resize(id + 1, DevBitmap{nullptr, 0, 0});
    r->bitmap_table[id] = DevBitmap{pixels, w, h};
    r->bitmap_table_dirty = true;
}
// A one-entry filter list over the texels of a registered bitmap, in place (swfr_blur_bitmap, swfr_convolve_bitmap): planned from
// texels (filter_plan.hpp), run behind everything queued on the handle and waited for
int filter_bitmap(swfr_renderer* r, uint32_t bitmap_id, const swfr_filter& entry, const swfr_kernel* kernel) {
    return guarded(r, [&]() {
        const auto bit = r->bitmaps.find(bitmap_id);
        if (bit == r->bitmaps.end() || !bit->second.pixels) return fail(r, SWFR_ERR_NOT_FOUND, "BitmapNotFound");
        const DeviceBitmap& bm = bit->second;
        wait_all_streams(r);
        const FilterPlan plan = plan_filters(&entry, 1, Source::Texels);
        if (plan.uses[T1]) r->blur_scratch.reserve(size_t(bm.width) * bm.height);
        uint32_t* const bufs[4] = {nullptr, bm.pixels, r->blur_scratch.ptr, nullptr};
        run_filter_plan(r->stream, plan, &entry, kernel, bufs, bm.width, bm.height);
        HIP_CHECK(hipStreamSynchronize(r->stream));
        bitmap_slot_has_new_texels(r, bitmap_id, bm.pixels, bm.width, bm.height, true);
        return int(SWFR_OK);
    });
}

// ---- swfr_render_resident: frames of the resident scene, queued back to back over the frame sets and waited for.  What a call's steps share:
struct ResidentCall {
    uint32_t frames, n_sets, used_sets;           // used_sets: the sets that render a frame of this call (the others hold an older frame's counters)
    uint32_t stride, first_timed, n_timed;        // per-kernel events on every stride-th frame from first_timed on: n_timed frames
    uint32_t rb; bool batched;                    // frames per launch; more than one, so no frame is timed
    uint32_t last_set;                            // the set of the call's last frame
    int64_t last_on[4] = {-1, -1, -1, -1};        // per frame set's stream: the last launch of this call it carries (none: -1)
    uint32_t last_parity[4] = {0, 0, 0, 0};       // per frame set: the descriptor its last frame of this call ran with (its counters are that one's)
    hipEvent_t begin, end, *join;                 // behind the timed frames' events in swfr_renderer::ev
};
// Whether a call of several frames per launch takes the fused chain, two launches a frame (ChainFrames::next; DESIGN.md 6.1, "k2_bin of
// the next frame in the row launch") -- only what k2_rows_ahead_b was built for; every other call keeps the three-launch chain.
bool bins_ahead(const swfr_renderer* r, const swfr_renderer::Scene& sc, const LaunchPlan& plan) {
    return r->bin_ahead                                               // not under SWFR_BIN_AHEAD=0
        && sc.frames_ahead                                            // the upload made parity-1 descriptors: into every set, antialiased, not one band of several (upload2)
        && sc.slow_verified                                           // not the scene's first call: what it needs of the queued-row kernels is not known yet
        && !plan.run_slow                                             // not a scene with queued rows
        && !plan.linear_grid                                          // not one with pixman-linear pieces
        && !r->mono                                                   // not an aliased handle
        && !r->bin_threads                                            // not under SWFR_BIN_THREADS: the fused kernel has the plan's own k2_bin instance alone
        && !r->use_graphs                                             // not under SWFR_GRAPHS
        && !rows_wide_instance(plan.max_path_edges, plan.rows_wide);  // not a path of more than 32 edges, nor SWFR_ROWS_WIDE: the narrow row kernel alone
}
// 1. the frame sets, the timed frames and their events, the frames per launch
ResidentCall plan_resident_call(swfr_renderer* r, uint32_t frames) {
    ResidentCall C{};
    C.frames = frames; C.n_sets = frames > 1 ? sets_of_scene(r) : 1u; C.used_sets = std::min(frames, C.n_sets);
    C.stride = r->event_stride < 1 ? 1u : uint32_t(r->event_stride);
    if (frames < 64 && !r->event_stride_given) C.stride = std::min(C.stride, 8u);   // (a short run still gets two or three frames with per-kernel times, unless SWFR_EVENT_STRIDE says otherwise)
    C.first_timed = std::min(C.stride / 2, frames - 1);               // (not frame 0: the first frames run before the pipeline is full)
    C.n_timed = (frames - C.first_timed + C.stride - 1) / C.stride;
    // events: four per timed frame (indexed by the timed frame's ordinal), then begin, end and the joins; created once, never inside
    // a later call's timed region unless it times more frames than any call before
    for (hipEvent_t e = nullptr; r->ev.size() < size_t(C.n_timed) * 4 + 5; r->ev.push_back(e)) HIP_CHECK(hipEventCreate(&e));
    C.begin = r->ev[size_t(C.n_timed) * 4]; C.end = r->ev[size_t(C.n_timed) * 4 + 1]; C.join = &r->ev[size_t(C.n_timed) * 4 + 2];
    // Frames per launch: the frame sets are cut into groups of `rb` (their descriptors are contiguous), a group's frames are one launch
    // per kernel (blockIdx.y = frame) on the group's first stream, and the groups alternate -- a third of the host's launches per
    // frame (three launches take the host about as long as a frame takes the GPU) and the GPU still has two streams to overlap.
    // Only without per-kernel events (a timed frame is launched alone).
    C.rb = (r->resident_batch >= 2 && C.stride > frames) ? uint32_t(r->resident_batch) : 1u;
    while (C.rb > 1 && (C.rb > C.n_sets || C.n_sets % C.rb != 0)) --C.rb;
    C.batched = C.rb > 1 && frames >= 2;
    C.last_set = (frames - 1) % C.n_sets;
    return C;
}
// 2. all frames are queued back to back, rotating over the frame sets; events bracket every kernel on the stream a timed frame runs on
void queue_resident_frames(swfr_renderer* r, const swfr_renderer::Scene& sc, ResidentCall& C) {
    const uint32_t frames = C.frames, n_sets = C.n_sets, rb = C.rb;
    // (no clearing of the counters here: k2_bin zeroes its frame's counters itself)
    // every frame set's graph exists before the first launch: a call never captures one between two frames (a short first call --
    // a warm-up of a few frames -- would otherwise leave the capture of the sets it launched with events to the next call)
    const bool graphs = frames > 1 && r->use_graphs && sc.slow_verified;
    if (graphs && !(r->resident_batch >= 2 && C.stride > frames))
        for (uint32_t k = 0; k < n_sets; ++k) ensure_frame_graph(r, sc, r->fs[k]);
    HIP_CHECK(hipEventRecord(C.begin, r->stream));
    order_frames_behind_pending_read(r);
#ifdef SWFR_BEGIN_WAIT
    for (uint32_t k = 1; k < n_sets; ++k) HIP_CHECK(hipStreamWaitEvent(r->fs[k].stream, C.begin, 0));
#endif
    // (the other sets' streams are not ordered behind the begin event: every call ends with all streams joined and waited for, an upload
    //  orders them behind its copy, and three more API calls before the first launch cost a short call a microsecond per frame)
    r->last_ahead_launches = 0;
    if (C.batched) {
        const uint32_t groups = n_sets / rb, launches = (frames + rb - 1) / rb;
        const LaunchPlan plan = plan_of(r, sc);                // (as a frame of its own, with the tile pass in its default shape unless SWFR_TILES_GRID caps it)
        // The fused chain: a group's launch k of the call runs with the descriptors of parity k & 1 (k2_bin first when k == 0) and its row
        // launch bins the group's next frames into the other parity's -- but for the group's last launch of the call: nothing is binned that
        // no row pass reads, so each strip_cost copy sees one row pass between two clears, across calls and the routes that use parity 0 alone.
        const bool ahead = bins_ahead(r, sc, plan);
        uint32_t gi = 0;
        for (uint32_t f = 0; f < frames; f += rb, ++gi) {
            const uint32_t g = gi % groups, cnt = std::min(rb, frames - f);
            ChainFrames cf{sc.frames_dev + g * rb, cnt};
            if (ahead) {
                const uint32_t parity = (gi / groups) & 1u;
                if (parity) cf.cur = sc.frames_ahead + g * rb;
                cf.binned = gi >= groups;                       // (all but the prologue: the group's launch before this one binned these frames)
                if (gi + groups < launches) { cf.next = (parity ? sc.frames_dev : sc.frames_ahead) + g * rb; cf.n_next = std::min(rb, frames - (f + groups * rb)); }
                for (uint32_t k = 0; k < cnt; ++k) C.last_parity[g * rb + k] = parity;
            }
            launch_chain(r, r->fs[g * rb].stream, cf, plan, nullptr, nullptr);
            C.last_set = g * rb + cnt - 1;
            C.last_on[g * rb] = int64_t(gi);
        }
    } else for (uint32_t f = 0; f < frames; ++f) {
        swfr_renderer::FrameSet& F = r->fs[f % n_sets];
        const bool timed = f >= C.first_timed && (f - C.first_timed) % C.stride == 0;   // per-kernel events on every stride-th frame (each costs a queue packet)
        if (!timed && graphs) { ensure_frame_graph(r, sc, F); HIP_CHECK(hipGraphLaunch(F.graph_exec, F.stream)); }
        else launch_frame(r, sc, F, nullptr, timed ? &r->ev[size_t((f - C.first_timed) / C.stride) * 4] : nullptr, n_sets > 1 && frames > 1);
        C.last_on[f % n_sets] = int64_t(f);
    }
}
// 3. the other streams join the handle's, the counters are copied behind the last kernel, and every stream is waited for
void join_resident_streams(swfr_renderer* r, ResidentCall& C) {
    for (uint32_t k = 1; k < C.n_sets; ++k) {              // (only the streams that carried something join)
        if (C.last_on[k] < 0) continue;
        HIP_CHECK(hipEventRecord(C.join[k - 1], r->fs[k].stream));
        HIP_CHECK(hipStreamWaitEvent(r->stream, C.join[k - 1], 0));
    }
    HIP_CHECK(hipEventRecord(C.end, r->stream));
    HIP_CHECK(hipGetLastError());
    // the counters of every set come back through pinned memory behind the last kernel: one synchronisation for everything
    // (a set whose last frame ran with its parity-1 descriptor left that frame's counters four sets further on: all eight come back)
    queue_counters(r->stream, pinned_counters(r), r->d_counters.ptr, r->last_ahead_launches ? 8u : C.used_sets);
    // The other sets' streams are waited for too, in the order their last frames finish: the runtime then knows them idle, and a
    // hipDeviceSynchronize behind this call (torch.cuda.synchronize()) costs 3 us instead of 47 (it drains every stream it has not seen
    // idle, 12 us apiece).  All but the last of these waits return while the GPU is still at the call's last frames.
    for (;;) {
        int pick = -1;
        for (uint32_t k = 1; k < C.n_sets; ++k)
            if (C.last_on[k] >= 0 && (pick < 0 || C.last_on[k] < C.last_on[pick])) pick = int(k);
        if (pick < 0) break;
        if (r->fs[pick].stream) HIP_CHECK(hipStreamSynchronize(r->fs[pick].stream));
        C.last_on[pick] = -1;
    }
    HIP_CHECK(hipStreamSynchronize(r->stream));
}
// ... and the call's times: swfr_last_timing but for n_records
void read_resident_times(swfr_renderer* r, const swfr_renderer::Scene& sc, const ResidentCall& C) {
    float setup_ms = 0, rows_ms = 0, tiles_ms = 0, total_ms = 0;
    uint32_t timed_frames = 0;
    for (uint32_t f = C.batched ? C.frames : C.first_timed; f < C.frames; f += C.stride, ++timed_frames) {      // (frames per launch: no per-kernel events)
        hipEvent_t* e = &r->ev[size_t(timed_frames) * 4];
        float a = 0, b = 0, c = 0;
        HIP_CHECK(hipEventElapsedTime(&a, e[0], e[1]));
        HIP_CHECK(hipEventElapsedTime(&b, e[1], e[2]));
        HIP_CHECK(hipEventElapsedTime(&c, e[2], e[3]));
        setup_ms += a; rows_ms += b; tiles_ms += c;
    }
    HIP_CHECK(hipEventElapsedTime(&total_ms, C.begin, C.end));
    r->timing = swfr_timing{total_ms, setup_ms, rows_ms, tiles_ms, C.frames, sc.dims.n_edges, sc.dims.n_paths, sc.dims.n_rows, 0, timed_frames};
}
// 4. set k's counters of its last frame of the call: error flags, queued rows, queue passes, records
const uint32_t* set_counters(const swfr_renderer* r, const ResidentCall& C, uint32_t k) {
    return r->h_counters + size_t(C.last_parity[k] ? 4 + k : k) * COUNTER_WORDS;
}
// 5. what the scene needs of the queued-row kernels, from the frames' own counters: kept for its next frames and as the next scene's guess.
// False: the launches were not enough for that guess -- rows were left in a queue nobody read, and the scene is set to launch everything
bool learn_queued_rows(swfr_renderer* r, const ResidentCall& C) {
    swfr_renderer::Scene& sc = r->scn[0];
    uint32_t slow = 0, huge = 0, passes = 1;
    for (uint32_t k = 0; k < C.used_sets; ++k) {
        const uint32_t* c = set_counters(r, C, k);
        slow |= c[C2_SLOW]; huge |= c[C2_HUGE];
        for (uint32_t q = 1; q < SLOW_PASSES; ++q)
            if (c[C2_SLOWQ + q] | c[C2_HUGEQ + q]) { passes = std::max(passes, q + 1); huge |= c[C2_HUGEQ + q]; }
    }
    const bool short_launch = (sc.slow_state == 1 && slow) || (sc.slow_state == 2 && huge) || passes > sc.slow_passes;
    sc.slow_state = slow == 0 ? 1 : (huge == 0 ? 2 : 0); sc.slow_passes = passes;     // what the next frames of this resident scene can skip
    r->hint_slow_state = sc.slow_state; r->hint_slow_passes = passes;
    sc.slow_verified = !short_launch;
    if (short_launch) { sc.slow_state = 0; sc.slow_passes = SLOW_PASSES; }
    return !short_launch;
}

int render_resident(swfr_renderer* r, uint32_t frames) {
    if (!r->has_device) return fail(r, SWFR_ERR_NO_DEVICE, "host-only handle cannot rasterize");
    if (!r->scene_ready) return fail(r, SWFR_ERR_INVALID, "no scene uploaded");
    if (frames == 0) frames = 1;
    if (frames > 1 && r->scene_from_builder && r->sets_ready < sets_wanted(r)) {
        // swfr_render prepared one frame set for its one frame; several frames of the same scene rotate over all of them
        const int rc = upload2(r, 0, true, builder_view(r), nullptr, true);
        if (rc != SWFR_OK) return rc;
    }
    if (frames > 1 && r->use_graphs && !r->scn[0].slow_verified) {
        // which queued-row kernels the scene needs is learnt from one blocking frame, so that the graphs of the frames behind it
        // are captured once (with exactly those kernels) and a later call finds them ready
        const int rc = render_resident(r, 1);
        if (rc != SWFR_OK) return rc;
        --frames;
    }
    if (frames > 4096) frames = 4096;
    const swfr_renderer::Scene& sc = r->scn[0];
    ResidentCall C = plan_resident_call(r, frames);
    queue_resident_frames(r, sc, C);
    join_resident_streams(r, C);
    r->fb_cur = r->n_targets ? r->targets[C.last_set % r->n_targets] : r->fs[C.last_set].d_fb.ptr;
    read_resident_times(r, sc, C);
    uint32_t counters[COUNTER_WORDS];
    std::memcpy(counters, set_counters(r, C, 0), sizeof counters);
    for (uint32_t k = 1; k < C.used_sets; ++k)             // (set 0's counts, every set's error and limit flags)
        for (uint32_t w : {uint32_t(C2_ERROR), uint32_t(C2_TIE_PAIRTEST_SKIPPED), uint32_t(C2_TIE_SORT_OVERFLOW), uint32_t(C2_TIE_DEPTH)})
            counters[w] |= set_counters(r, C, k)[w];
    r->fb_valid = learn_queued_rows(r, C);
    if (!r->fb_valid) return render_resident(r, frames);   // (a short launch: the frames are not valid, and are rendered again with everything)
    for (uint32_t h = 0; h < C2_HEADS; ++h) r->timing.n_records += counters[C2_HEAD + h];     // cells of the last frame of set 0
    return check_counters(r, counters);
}

// The blurred, shadowed and filtered layers of the frame the builder has just built, before the frame itself (swfr_render): sub-frame k
// is validated, uploaded and rendered as an ordinary frame, once, and its filter list (a blurred or shadowed layer's has one entry) is
// planned from the framebuffer into texture k of the pool (filter_plan.hpp; DESIGN.md, "Filter lists") and run.  Everything runs on
// the handle's stream, behind the sub-frame's kernels (render_resident returns with every stream idle), and is waited for once per
// layer: the builder's arrays and the framebuffer are free for the next sub-frame, and for the parent.
int render_blur_layers(swfr_renderer* r) {
    const auto& layers = r->builder->layers();
    if (r->cfg.band_count > 1) throw StatusError{SWFR_ERR_NOT_IMPLEMENTED, "NotImplementedBlurBands"};
    const size_t n = size_t(r->width) * r->height;
    r->blur_table.assign(layers.size(), DevBitmap{nullptr, 0, 0});
    // scene slot 0 and the framebuffer are about to hold sub-frames: neither is "the scene" or "the frame" until the parent is up,
    // whichever way this function is left (upload2 and render_resident set the flags again for each sub-frame: cleared behind them)
    struct Invalidate { swfr_renderer* r; ~Invalidate() { r->scene_ready = false; r->fb_valid = false; r->scene_from_builder = false; } } invalidate{r};
    r->scene_ready = false; r->fb_valid = false;
    for (size_t k = 0; k < layers.size(); ++k) {
        const BlurLayer& B = layers[k];
        const SceneView sv{B.edges.data(), B.edges.size(), B.paths.data(), B.paths.size(), B.styles.data(), B.styles.size()};
        r->blur_tex[k].reserve(n);
        uint32_t* const tex = r->blur_tex[k].ptr;
        if (B.paths.empty()) {                                 // nothing drawn: the group is clear, and so is its blur
            HIP_CHECK(hipMemsetAsync(tex, 0, n * 4, r->stream));
        } else {
            validate_scene(r, sv);
            int rc = upload2(r, 0, false, sv, nullptr, true);
            if (rc == SWFR_OK) rc = render_resident(r, 1);
            if (rc != SWFR_OK) return rc;
            const FilterPlan plan = plan_filters(B.filters, B.n_filters, Source::Framebuffer);
            if (plan.uses[T1]) r->blur_scratch.reserve(n);            // (a lone box of 1 x 1 runs no pass: the capture is the texture)
            if (plan.uses[T2]) r->shadow_scratch.reserve(n);
            uint32_t* const bufs[4] = {r->fb_cur ? r->fb_cur : r->fs[0].d_fb.ptr, tex, r->blur_scratch.ptr, r->shadow_scratch.ptr};
            run_filter_plan(r->stream, plan, B.filters, B.kernels, bufs, r->width, r->height);
        }
        HIP_CHECK(hipStreamSynchronize(r->stream));
        r->blur_table[k] = DevBitmap{tex, r->width, r->height};
    }
    return SWFR_OK;
}

// swfr_render; allow_blur: the route draws blurred layers (the sequence entries refuse them)
int render_stage(swfr_renderer* r, const swfr_stage* stage, bool allow_blur) {
    if (!r || !stage) return fail(r, SWFR_ERR_INVALID, "null argument");
    if (!r->has_device) return fail(r, SWFR_ERR_NO_DEVICE, "host-only handle cannot rasterize");
    ++r->cx_epoch;
    return guarded(r, [&]() {
        using clk = std::chrono::steady_clock;
        auto ms = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
        const auto t0 = clk::now();
        r->builder->build(*stage);
        const auto tb = clk::now();
        r->blur_table.clear();
        const bool blurred = !r->builder->layers().empty();
        if (blurred) {
            if (!allow_blur) refuse_blur_route(r);
            const int rc = render_blur_layers(r);
            if (rc != SWFR_OK) return rc;
        }
        validate_scene(r, builder_view(r), blurred);
        // (one frame set: this frame is rendered alone; the builder's edges carry their path index)
        int rc = upload2(r, 0, false, builder_view(r), nullptr, true);
        const auto t2 = clk::now();
        if (rc != SWFR_OK) return rc;
        rc = render_resident(r, 1);
        const auto t3 = clk::now();
        swfr_path_timing& pt = r->path_timing;
        // (upload_host_ms takes in the blurred layers' sub-frames, rendered above: swfr.h)
        pt.build_ms = ms(t0, tb); pt.upload_host_ms = ms(tb, t2); pt.device_ms = r->timing.total_ms; pt.total_ms = ms(t0, t3);
        pt.h2d_bytes = r->scn[0].arena.used; pt.h2d_ms = 0;
        if (r->scn[0].arena.copy_begin) {
            float h = 0;
            if (hipEventElapsedTime(&h, r->scn[0].arena.copy_begin, r->scn[0].arena.copy_end) == hipSuccess) pt.h2d_ms = h;
        }
        return rc;
    });
}

// A batch of different frames (BASELINE config 3: 256 morph ratios): frame i is built on the host, uploaded into the scene slot
// of frame set i mod n and rasterized on that set's stream straight into device_dst + i * frame_stride, while the host already
// builds frame i+1.  Nothing waits for the GPU until the end (a scene slot's pinned staging buffer is reused only after its
// previous H2D copy has completed).
// swfr_render_batch with a device destination: the frames are rendered in groups of SWFR_BATCH_FRAMES (default 64) by
// one launch per kernel and group (blockIdx.y = frame of the group, every frame with its own descriptor, tables and buffers), so a
// batch of small frames -- the 256 ratios of a morph shape -- fills the GPU instead of paying a launch chain per frame.  Two groups
// alternate: the host builds group g + 1 (scene walk, flattening, layout) while the GPU rasterizes group g.
int render_batch2(swfr_renderer* r, const swfr_stage* stages, uint32_t n, void* device_dst, size_t frame_stride) {
    // a frame of the group being built: the builder's arrays (the builder goes on to the next frame), what prepare_frame made of them
    struct FrameData { std::vector<swfr_edge> e; std::vector<swfr_path> p; std::vector<swfr_style> s; FrameScratch scratch; SceneLayout L; SceneView a; FrameDims dims; };
    static thread_local std::vector<FrameData> fd;
    // frames per group: SWFR_BATCH_FRAMES at most; a call with fewer frames is still cut into four groups, so that building group
    // g + 1 overlaps rasterizing group g, as long as a group keeps enough pixels (32 Mpx: four 4K frames, thirty-two 1024x1024 ones)
    // for one launch per kernel to fill the GPU
    const uint32_t fill = uint32_t((size_t(32) << 20) / std::max<size_t>(size_t(r->width) * r->height, 1)) + 1;
    const uint32_t B = std::min(uint32_t(std::max(1, r->batch_frames)), std::max((n + 3) / 4, fill));
    const uint32_t tiles_x = (r->width + TILE_W - 1) / TILE_W;
    using clk = std::chrono::steady_clock;
    auto ms_since = [](clk::time_point a) { return std::chrono::duration<double, std::milli>(clk::now() - a).count(); };
    double t_build = 0, t_wait = 0, t_stage = 0, t_launch = 0;
    const bool trace = std::getenv("SWFR_BATCH_TRACE") != nullptr;          // host time per stage of the call, to stderr
    if (r->bitmap_table_dirty) {
        r->d_bitmap_table.reserve(r->bitmap_table.size());
        if (!r->bitmap_table.empty()) HIP_CHECK(hipMemcpy(r->d_bitmap_table.ptr, r->bitmap_table.data(), r->bitmap_table.size() * sizeof(DevBitmap), hipMemcpyHostToDevice));
        r->bitmap_table_dirty = false;
    }
    int rc = SWFR_OK;
    double device_ms = 0;                                   // kernels only, summed over the groups (they do not overlap each other much)
    uint32_t gi = 0;
    uint32_t pend[2] = {0, 0};                              // per group: the frames of its launch whose counters have not been checked
    auto finish_group = [&](int g) {                        // waits for a group's launches and checks its frames' counters
        auto& G = r->groups[g];
        if (!pend[g]) return;
        HIP_CHECK(hipStreamSynchronize(G.stream));
        float ms = 0;
        if (hipEventElapsedTime(&ms, G.ev_begin, G.ev_end) == hipSuccess) device_ms += ms;
        rc = check_frames(r, G.h_counters, pend[g], rc);
        pend[g] = 0;
    };
    try {
        for (uint32_t first = 0; first < n && rc == SWFR_OK; first += B, ++gi) {
            const uint32_t cnt = std::min(B, n - first);
            const int g = int(gi & 1);
            auto& G = r->groups[g];
            if (!G.stream) HIP_CHECK(hipStreamCreateWithFlags(&G.stream, hipStreamNonBlocking));
            // ---- host: build the group's frames (the other group is being rasterized meanwhile)
            if (fd.size() < cnt) fd.resize(cnt);
            size_t arena_bytes = pad256(cnt * sizeof(Frame2)) + 4096, work_bytes = 0, cls_bytes = 0;
            // the group's plan: the running maximum over its frames' layouts.  Nothing renders a frame of a batch again: k2_bin always prepares the queued rows, their kernels run
            // -- in the grids of frames that share the GPU, with every pass -- whenever a frame has row chunks; the tile pass keeps its default shape whatever SWFR_TILES_GRID says
            LaunchPlan plan{};
            plan.slow_kernels = 1u; plan.grid_slow = 256u; plan.grid_huge = 64u; plan.slow_passes = SLOW_PASSES; plan.tiles_grid = ~0u;
            auto t0 = clk::now();
            for (uint32_t k = 0; k < cnt; ++k) {
                FrameData& F = fd[k];
                r->builder->build(stages[first + k]);
                refuse_blur_route(r);
                validate_scene(r, builder_view(r));
                F.e = r->builder->edges(); F.p = r->builder->paths(); F.s = r->builder->styles();
                F.a = prepare_frame(r, SceneView{F.e.data(), F.e.size(), F.p.data(), F.p.size(), F.s.data(), F.s.size()}, G.stream, false, F.scratch, F.L);
                F.dims = FrameDims::of_layout(F.L, F.a.n_edges, F.a.n_paths);
                arena_bytes += scene_arena_bytes(F.L, F.a);
                work_bytes += frame_work_bytes(F.dims); cls_bytes += pad256(cls_region_bytes(F.dims, tiles_x));
                merge_bounds(plan, plan_bounds(F.L, F.a.n_edges, F.a.n_paths));
            }
            plan.run_slow = plan.max_chunks != 0;
            plan.bin_threads = bin_threads_of(r, plan.max_paths, true);     // (over the frames of the launch; the other group's launch runs beside it)
            t_build += ms_since(t0); t0 = clk::now();
            // ---- this group's previous use must be over before its staging and device buffers are rewritten
            finish_group(g);
            t_wait += ms_since(t0); t0 = clk::now();
            if (rc != SWFR_OK) break;
            G.arena.begin(arena_bytes);
            const uint8_t* work_before = G.work.ptr;
            G.work.reserve(work_bytes + 4096); G.cls.reserve(cls_bytes + 4096);
            if (G.work.ptr != work_before) HIP_CHECK(hipMemsetAsync(G.work.ptr, 0, G.work.cap, G.stream));      // (fresh memory: the strip costs start at zero)
            HIP_CHECK(hipMemsetAsync(G.cls.ptr, 0, cls_bytes, G.stream));                                        // class bytes outside the paths' rectangles
            if (G.h_counters_cap < cnt) {
                if (G.h_counters) (void)hipHostFree(G.h_counters);
                HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&G.h_counters), size_t(B) * COUNTER_WORDS * sizeof(uint32_t), hipHostMallocDefault));
                G.h_counters_cap = B;
            }
            std::vector<Frame2> fr(cnt);
            uint8_t *w = G.work.ptr, *c = G.cls.ptr;
            for (uint32_t k = 0; k < cnt; ++k) {
                const FrameData& F = fd[k];
                Frame2& f = fr[k];
                std::memset(&f, 0, sizeof f);
                push_scene(G.arena, F.L, F.a, f);
                fill_frame_sizes(r, F.L, F.a, f);
                f.src.bitmaps = r->d_bitmap_table.ptr;
                place_frame(f, F.dims, tiles_x, w, c);
                f.strip_order = 0;                             // (a frame's buffers held another frame before: no cost history to order by)
                f.fb = reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(device_dst) + size_t(first + k) * frame_stride);
            }
            const Frame2* frames_dev = static_cast<Frame2*>(G.arena.push(fr.data(), cnt * sizeof(Frame2)));
            G.arena.flush(G.stream);
            t_stage += ms_since(t0); t0 = clk::now();
            if (!G.ev_begin) { HIP_CHECK(hipEventCreate(&G.ev_begin)); HIP_CHECK(hipEventCreate(&G.ev_end)); }
            HIP_CHECK(hipEventRecord(G.ev_begin, G.stream));
            launch_chain(r, G.stream, {frames_dev, cnt}, plan, nullptr, nullptr);
            HIP_CHECK(hipEventRecord(G.ev_end, G.stream));
            queue_counters(G.stream, G.h_counters, fr.data(), cnt);
            HIP_CHECK(hipGetLastError());
            pend[g] = cnt;
            r->fb_cur = fr[cnt - 1].fb;
            t_launch += ms_since(t0);
        }
    } catch (...) {
        // a refused frame (a StatusError of the frame builder or the layout) or a failed HIP call while up to two groups still
        // write the caller's frames: they finish, and their counters are read, before the error reaches the caller (swfr.h)
        try {
            for (int g = 0; g < 2; ++g)
                if (r->groups[g].stream) HIP_CHECK(hipStreamSynchronize(r->groups[g].stream));   // (also a texel pass of the group being built)
            finish_group(0);
            finish_group(1);
        } catch (...) {}
        r->scene_ready = false;
        r->fb_valid = false; r->fb_cur = nullptr;
        throw;
    }
    auto t_end = clk::now();
    finish_group(0);
    finish_group(1);
    if (trace) std::fprintf(stderr, "[swfr] batch of %u frames in groups of %u: build+layout %.3f ms, waiting for a group's buffers %.3f, staging %.3f, launches %.3f, final wait %.3f, kernels %.3f\n",
                            n, B, t_build, t_wait, t_stage, t_launch, ms_since(t_end), device_ms);
    r->scene_ready = false;
    r->fb_valid = rc == SWFR_OK;
    r->timing = swfr_timing{float(device_ms), 0, 0, 0, n, 0, 0, 0, 0, 0};     // (swfr_last_timing: total_ms = the groups' kernel time)
    return rc;
}

// The resident scene as `per_launch` frames per kernel launch (blockIdx.y = frame, every frame with its own kernel-written buffers
// and its own framebuffer), `launches` times back to back on one stream: the GPU saturated by one scene -- what frames in flight
// approximate with streams.  Every frame recomputes everything from the raw edge list, as in swfr_render_resident.
int render_resident_batched(swfr_renderer* r, uint32_t per_launch, uint32_t launches, float* ms_out) {
    if (!r->has_device) return fail(r, SWFR_ERR_NO_DEVICE, "host-only handle cannot rasterize");
    if (!r->scene_ready) return fail(r, SWFR_ERR_INVALID, "no scene uploaded");
    if (per_launch == 0 || per_launch > 64 || launches == 0) return fail(r, SWFR_ERR_INVALID, "1..64 frames per launch, at least one launch");
    // which queued-row kernels the scene needs: from a blocking frame of the scene itself
    if (!r->scn[0].slow_verified) { const int rc = render_resident(r, 1); if (rc != SWFR_OK) return rc; }
    const swfr_renderer::Scene& sc = r->scn[0];
    const uint32_t B = per_launch, tiles_x = (r->width + TILE_W - 1) / TILE_W;
    const size_t n_px = size_t(r->width) * r->height;
    const FrameDims& dims = sc.dims;
    const size_t work_one = frame_work_bytes(dims), cls_one = pad256(cls_region_bytes(dims, tiles_x));
    const hipStream_t st = r->stream;
    r->fb_valid = false;                                       // (fb_cur may point into a buffer the next lines reallocate; set again below)
    r->fb_cur = nullptr;
    const uint32_t* rb_fb_before = r->rb_fb.ptr;
    r->rb_work.reserve(work_one * B + 4096); r->rb_cls.reserve(cls_one * B + 4096); r->rb_frames.reserve(B); r->rb_fb.reserve(n_px * B);
    // (a handle that owns only some tile-rows writes only those: the rest of a fresh framebuffer is cleared once, as upload2 does for d_fb)
    if (r->rb_fb.ptr != rb_fb_before) HIP_CHECK(hipMemsetAsync(r->rb_fb.ptr, 0, r->rb_fb.cap * sizeof(uint32_t), st));
    HIP_CHECK(hipMemsetAsync(r->rb_work.ptr, 0, work_one * B, st));           // (strip costs start at zero; class bytes outside the paths' rectangles)
    HIP_CHECK(hipMemsetAsync(r->rb_cls.ptr, 0, cls_one * B, st));
    std::vector<Frame2> fr(B);
    uint8_t *w = r->rb_work.ptr, *c = r->rb_cls.ptr;
    for (uint32_t k = 0; k < B; ++k) {
        Frame2& f = fr[k];
        f = sc.proto;
        place_frame(f, dims, tiles_x, w, c);
        f.fb = r->rb_fb.ptr + n_px * k;
    }
    HIP_CHECK(hipMemcpyAsync(r->rb_frames.ptr, fr.data(), B * sizeof(Frame2), hipMemcpyHostToDevice, st));
    HIP_CHECK(hipStreamSynchronize(st));                       // (fr is a local)
    if (!r->rb_ev[0]) { HIP_CHECK(hipEventCreate(&r->rb_ev[0])); HIP_CHECK(hipEventCreate(&r->rb_ev[1])); }
    // as a frame of its own, but the queued-row kernels in the grids of frames that share the GPU, and the tile pass in its default shape whatever SWFR_TILES_GRID says
    LaunchPlan plan = plan_of(r, sc);
    plan.grid_slow = 256u; plan.grid_huge = sc.slow_state == 2 ? 0u : 64u; plan.tiles_grid = ~0u;
    plan.bin_threads = bin_threads_of(r, plan.max_paths, B > 1);
    launch_chain(r, st, {r->rb_frames.ptr, B}, plan, nullptr, nullptr);    // warm-up: leaves a cost history for the strip order
    HIP_CHECK(hipEventRecord(r->rb_ev[0], st));
    for (uint32_t l = 0; l < launches; ++l) launch_chain(r, st, {r->rb_frames.ptr, B}, plan, nullptr, nullptr);
    HIP_CHECK(hipEventRecord(r->rb_ev[1], st));
    HIP_CHECK(hipGetLastError());
    std::vector<uint32_t> hc(size_t(B) * COUNTER_WORDS);
    queue_counters(st, hc.data(), fr.data(), B);
    HIP_CHECK(hipStreamSynchronize(st));
    float ms = 0;
    HIP_CHECK(hipEventElapsedTime(&ms, r->rb_ev[0], r->rb_ev[1]));
    if (ms_out) *ms_out = ms;
    r->fb_cur = fr[B - 1].fb;
    r->fb_valid = true;
    return check_frames(r, hc.data(), B, SWFR_OK, &sc);       // (a frame that queued rows for kernels this call did not launch is not valid)
}

int render_batch(swfr_renderer* r, const swfr_stage* stages, uint32_t n, void* device_dst, size_t frame_stride) {
    if (!r->has_device) return fail(r, SWFR_ERR_NO_DEVICE, "host-only handle cannot rasterize");
    if (n == 0) return SWFR_OK;
    if (device_dst && frame_stride < size_t(r->width) * r->height * 4) return fail(r, SWFR_ERR_INVALID, "frame stride smaller than a frame");
    if (device_dst && r->batch_frames > 1) return render_batch2(r, stages, n, device_dst, frame_stride);
    order_frames_behind_pending_read(r);                       // (frames without a device_dst land in the frame sets' own framebuffers)
    const uint32_t n_sets = sets_wanted(r);
    uint32_t* hc = nullptr;
    HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&hc), size_t(n) * COUNTER_WORDS * sizeof(uint32_t), hipHostMallocDefault));
    int rc = SWFR_OK;
    try {
        for (uint32_t i = 0; i < n; ++i) {
            const int k = int(i % n_sets);
            r->builder->build(stages[i]);
            refuse_blur_route(r);
            uint32_t* fb_dst = device_dst ? reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(device_dst) + size_t(i) * frame_stride) : nullptr;
            validate_scene(r, builder_view(r));
            rc = upload2(r, k, false, builder_view(r), fb_dst, true);   // (the builder's edges carry their path index)
            if (rc != SWFR_OK) break;
            // nothing renders a frame of a batch again: every frame launches all the queued-row kernels (upload2 seeds set 0 with what
            // the previous scene needed, a guess only render_resident checks against the frame's counters)
            r->scn[k].slow_state = 0; r->scn[k].slow_passes = SLOW_PASSES;
            swfr_renderer::FrameSet& F = r->fs[k];
            if (k > 0 && i < n_sets) HIP_CHECK(hipStreamSynchronize(r->stream));   // first use of the set: bitmap table etc. are in place
            launch_frame(r, r->scn[k], F, nullptr, nullptr, n_sets > 1 && n > 1);     // (the descriptor carries the frame's target)
            queue_counters(F.stream, hc + size_t(i) * COUNTER_WORDS, F.counters);
            r->fb_cur = fb_dst ? fb_dst : F.d_fb.ptr;
        }
        HIP_CHECK(hipGetLastError());
        for (uint32_t k = 0; k < n_sets; ++k)
            if (r->fs[k].stream) HIP_CHECK(hipStreamSynchronize(r->fs[k].stream));
    } catch (...) {
        // a refused frame: the frames queued before it, and their counter copies into hc, finish before hc is freed and the error
        // reaches the caller (swfr.h); none of them is the handle's image
        for (uint32_t k = 0; k < 4; ++k)
            if (r->fs[k].stream) (void)hipStreamSynchronize(r->fs[k].stream);
        (void)hipStreamSynchronize(r->stream);
        (void)hipHostFree(hc);
        r->scene_ready = false;
        r->fb_valid = false; r->fb_cur = nullptr;
        throw;
    }
    r->scene_ready = false;                 // scene 0 now holds some frame of the batch, not a scene the caller uploaded
    r->fb_valid = true;
    rc = check_frames(r, hc, n, rc);
    (void)hipHostFree(hc);
    return rc;
}

// Mapped read-back of the last frame: the framebuffer (or its un-premultiplied copy) goes to the handle's PINNED staging buffer by
// one asynchronous copy on the handle's stream behind the frame's kernels, and the caller reads it there (a pageable destination makes
// the runtime stage the copy through its own pinned pieces and a host memcpy: 2.3 ms for a 4K frame instead of 0.6).
int start_read(swfr_renderer* r, int premultiplied) {
    if (r->read_pending) { HIP_CHECK(hipEventSynchronize(r->read_done)); r->read_pending = false; }      // (an earlier read-back nobody waited for)
    const size_t n = size_t(r->width) * r->height, bytes = n * 4;
    const uint32_t* src = r->fb_cur ? r->fb_cur : r->fs[0].d_fb.ptr;
    if (!src) return fail(r, SWFR_ERR_INVALID, "no framebuffer");
    if (!premultiplied) {
        r->d_tmp.reserve(n);
        launch_unpremultiply(r->stream, src, r->d_tmp.ptr, n);
        src = r->d_tmp.ptr;
    }
    if (r->h_image_cap < bytes) {
        if (r->h_image) (void)hipHostFree(r->h_image);
        r->h_image = nullptr; r->h_image_cap = 0;
        HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&r->h_image), bytes, hipHostMallocDefault));
        r->h_image_cap = bytes;
    }
    if (!r->read_done) HIP_CHECK(hipEventCreateWithFlags(&r->read_done, hipEventDisableTiming));
    HIP_CHECK(hipMemcpyAsync(r->h_image, src, bytes, hipMemcpyDeviceToHost, r->stream));
    HIP_CHECK(hipEventRecord(r->read_done, r->stream));
    r->read_pending = true;
    return SWFR_OK;
}
int finish_read(swfr_renderer* r) {
    if (!r->read_pending) return fail(r, SWFR_ERR_INVALID, "no read-back in flight");
    HIP_CHECK(hipEventSynchronize(r->read_done));
    r->read_pending = false;
    return SWFR_OK;
}

// One frame of the resident scene queued on the next frame set in rotation and not waited for (swfr_wait): into the set's own target, or
// -- block_target, always launched as a frame that shares the GPU -- into the caller's block of the handle's tile-rows.
int render_resident_async(swfr_renderer* r, void* block_target, uint32_t* out_set) {
    if (!r->has_device) return fail(r, SWFR_ERR_NO_DEVICE, "host-only handle cannot rasterize");
    if (!r->scene_ready) return fail(r, SWFR_ERR_INVALID, "no scene uploaded");
    const BandShare bs = band_share(r);
    if (block_target && bs.stride != 1) return fail(r, SWFR_ERR_INVALID, "a block target needs a handle that owns one contiguous block of tile-rows");
    return guarded(r, [&]() {
        const uint32_t n_sets = sets_of_scene(r);
        const uint32_t k = r->async_next++ % n_sets;
        r->async_used |= 1u << k;
        if (!r->scn[0].slow_verified) { r->scn[0].slow_state = 0; r->scn[0].slow_passes = SLOW_PASSES; }   // (nothing checks an async frame's queues: launch everything unless a blocking frame of this scene has shown what it needs)
        // row y of the frame is row y - (first tile-row) * 16 of the block: the kernels address the frame, so they get the block's
        // address moved up by the rows above it (only the handle's own rows are ever written)
        uint32_t* fb_to = block_target ? static_cast<uint32_t*>(block_target) - size_t(bs.first) * TILE_H * r->width : nullptr;
        order_frames_behind_pending_read(r);
        launch_frame(r, r->scn[0], r->fs[k], fb_to, nullptr, block_target || n_sets > 1);
        HIP_CHECK(hipGetLastError());
        r->fb_cur = block_target ? nullptr : (r->n_targets ? r->targets[k % r->n_targets] : r->fs[k].d_fb.ptr);
        if (block_target) r->fb_valid = false;                 // (the frame is the caller's: nothing to read back from the handle)
        if (out_set) *out_set = k;
        return int(SWFR_OK);
    });
}

// The skeleton of the swfr_debug_time_* probes, on the handle's stream: the device buffers are allocated (and set to their fill byte),
// the events created, `warm_up` run once; then each phase's launch is queued `reps` times between two events, the last event waited
// for, and *ms of each phase is the time of one of its launches.  The buffers and events are freed behind a wait for the stream,
// whether or not something threw.
struct ProbeBuffer { uint32_t** ptr; size_t bytes; int fill; };      // *ptr: nullptr on entry; fill < 0: left as allocated
struct ProbePhase { std::function<void()> launch; float* ms; };
int time_phases(swfr_renderer* r, uint32_t reps, std::initializer_list<ProbeBuffer> buffers, const std::function<void()>& warm_up, std::initializer_list<ProbePhase> phases) {
    std::vector<hipEvent_t> e(phases.size() + 1, nullptr);
    std::exception_ptr failure;
    try {
        for (const ProbeBuffer& b : buffers) HIP_CHECK(hipMalloc(reinterpret_cast<void**>(b.ptr), b.bytes));
        for (const ProbeBuffer& b : buffers) if (b.fill >= 0) HIP_CHECK(hipMemsetAsync(*b.ptr, b.fill, b.bytes, r->stream));
        for (auto& x : e) HIP_CHECK(hipEventCreate(&x));
        warm_up();
        HIP_CHECK(hipEventRecord(e[0], r->stream));
        for (size_t k = 0; k < phases.size(); ++k) {
            for (uint32_t i = 0; i < reps; ++i) phases.begin()[k].launch();
            HIP_CHECK(hipEventRecord(e[k + 1], r->stream));
        }
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipEventSynchronize(e.back()));
        for (size_t k = 0; k < phases.size(); ++k) HIP_CHECK(hipEventElapsedTime(phases.begin()[k].ms, e[k], e[k + 1]));
        for (const ProbePhase& ph : phases) *ph.ms /= float(reps);
    } catch (...) {
        failure = std::current_exception();
    }
    (void)hipStreamSynchronize(r->stream);
    for (const ProbeBuffer& b : buffers) if (*b.ptr) (void)hipFree(*b.ptr);
    for (auto& x : e) if (x) (void)hipEventDestroy(x);
    if (failure) std::rethrow_exception(failure);
    return SWFR_OK;
}

// (swfr_last_error(NULL): why this thread's last swfr_create refused a flag combination, if it did)
thread_local const char* create_error = nullptr;

// a caller's device address or stride that every kernel takes as uint32_t words
inline bool word_aligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0u; }
inline bool word_aligned(size_t bytes) { return (bytes & 3u) == 0u; }

}  // namespace

extern "C" {
#pragma GCC visibility push(default)

uint32_t swfr_abi_version(void) { return SWFR_ABI_VERSION; }

const char* swfr_last_error(const swfr_renderer* r) { return r ? r->error.c_str() : (create_error ? create_error : "null handle"); }

int swfr_create(uint32_t width, uint32_t height, const swfr_config* cfg, swfr_renderer** out) {
    if (!out) return SWFR_ERR_INVALID;
    *out = nullptr;
    if (width == 0 || height == 0 || width > 32768 || height > 32768) return SWFR_ERR_INVALID;
    std::unique_ptr<swfr_renderer> r(new (std::nothrow) swfr_renderer);
    if (!r) return SWFR_ERR_CAPACITY;
    r->width = width;
    r->height = height;
    if (cfg) r->cfg = *cfg;
    if (r->cfg.band_count > 1 && r->cfg.band_index >= r->cfg.band_count) return SWFR_ERR_INVALID;
    r->mono = (r->cfg.flags & SWFR_FLAG_ANTIALIAS_NONE) != 0;
    create_error = nullptr;
    // (aliased, every span is a piece of its own for pixman's linear ramp: validate_scene)
    if (r->mono && (r->cfg.flags & SWFR_FLAG_LINEAR_PIXMAN)) { create_error = "NotImplementedAliasedPixmanLinear"; return SWFR_ERR_NOT_IMPLEMENTED; }
    r->builder.reset(new FrameBuilder(width, height, (r->cfg.flags & SWFR_FLAG_EVEN_ODD) != 0, r->mono, (r->cfg.flags & SWFR_FLAG_LINEAR_PIXMAN) != 0,
                                        (r->cfg.flags & SWFR_FLAG_ALPHA_MODES) != 0));
    if (const char* fl = std::getenv("SWFR_FAST_LIMIT")) r->fast_limit = std::atoi(fl);
    if (const char* tg = std::getenv("SWFR_TILES_GRID")) r->tiles_grid = std::atoi(tg);
    if (const char* bt = std::getenv("SWFR_BIN_THREADS")) { const int v = std::atoi(bt); r->bin_threads = v == int(BIN_THREADS_SMALL) || v == int(BIN_THREADS_LARGE) ? v : 0; }
    if (const char* ts = std::getenv("SWFR_TILES_SHADERS")) r->tiles_shaders = std::min(std::max(std::atoi(ts), 0), 7);
    if (const char* rw = std::getenv("SWFR_ROWS_WIDE")) r->rows_wide = std::atoi(rw) != 0;
    if (const char* bf = std::getenv("SWFR_BATCH_FRAMES")) r->batch_frames = std::max(1, std::atoi(bf));
    if (const char* cr = std::getenv("SWFR_CHUNK_ROWS")) r->force_chunk_rows = std::atoi(cr);
    if (const char* so = std::getenv("SWFR_STRIP_ORDER")) r->strip_order = std::atoi(so);
    if (const char* fi = std::getenv("SWFR_FRAMES_IN_FLIGHT")) r->in_flight = std::atoi(fi);
    if (const char* es = std::getenv("SWFR_EVENT_STRIDE")) { r->event_stride = std::atoi(es); r->event_stride_given = true; }
    if (const char* ug = std::getenv("SWFR_GRAPHS")) r->use_graphs = std::atoi(ug);
#ifdef SWFR_EMU
    r->use_graphs = 0;                                              // (the emulator's runtime has no graphs)
#endif
    if (const char* rb = std::getenv("SWFR_RESIDENT_BATCH")) r->resident_batch = std::atoi(rb);
    if (const char* ba = std::getenv("SWFR_BIN_AHEAD")) r->bin_ahead = std::atoi(ba) != 0;
    if (const char* cm = std::getenv("SWFR_CXFORM_CACHE_MB")) r->cx_budget = size_t(std::max(0, std::atoi(cm))) << 20;
    if (r->cfg.device == SWFR_DEVICE_HOST_ONLY) {
        *out = r.release();
        return SWFR_OK;
    }
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return SWFR_ERR_NO_DEVICE;
    if (r->cfg.device < 0 || r->cfg.device >= count) return SWFR_ERR_NO_DEVICE;
    r->has_device = true;
    swfr_renderer* raw = r.get();
    const int rc = guarded(raw, [&]() {
        HIP_CHECK(hipStreamCreateWithFlags(&raw->stream, hipStreamNonBlocking));
        raw->fs[0].stream = raw->stream;
        // the frame sets' streams first: HIP deals streams onto a few hardware queues in creation order, and the sets must not share one
        for (uint32_t k = 1; k < sets_wanted(raw); ++k) HIP_CHECK(hipStreamCreateWithFlags(&raw->fs[k].stream, hipStreamNonBlocking));
        for (int i = 0; i < 4 * 32 + 5; ++i) { hipEvent_t e = nullptr; HIP_CHECK(hipEventCreate(&e)); raw->ev.push_back(e); }   // (so that no render call has to create its timing events inside somebody's timed region)
        raw->fs[0].d_fb.reserve(size_t(width) * height);
        HIP_CHECK(hipMemsetAsync(raw->fs[0].d_fb.ptr, 0, size_t(width) * height * 4, raw->stream));
        raw->d_counters.reserve(8 * COUNTER_WORDS);
        raw->fs[0].counters = raw->d_counters.ptr;
        HIP_CHECK(hipStreamSynchronize(raw->stream));
        return int(SWFR_OK);
    });
    if (rc != SWFR_OK) return rc;
    *out = r.release();
    return SWFR_OK;
}

void swfr_destroy(swfr_renderer* r) { delete r; }

int swfr_register_shape(swfr_renderer* r, const swfr_define_shape* tag, uint32_t* out_id) {
    if (!r || !tag || !out_id) return fail(r, SWFR_ERR_INVALID, "null argument");
    return guarded(r, [&]() {
        *out_id = r->builder->add_shape(decode_shape(*tag, false));
        return int(SWFR_OK);
    });
}

int swfr_register_morph_shape(swfr_renderer* r, const swfr_define_shape* tag, uint32_t* out_id) {
    if (!r || !tag || !out_id) return fail(r, SWFR_ERR_INVALID, "null argument");
    return guarded(r, [&]() {
        *out_id = r->builder->add_morph_shape(decode_shape(*tag, true));
        return int(SWFR_OK);
    });
}

int swfr_decode_x_swf_bmp(const uint8_t* data, size_t len, uint32_t* width, uint32_t* height, uint8_t* rgba, size_t rgba_cap) {
    if (!data || !width || !height) return SWFR_ERR_INVALID;
    try {
        std::vector<uint8_t> px;
        const XSwfBmpStatus st = decode_x_swf_bmp(data, len, *width, *height, px);
        if (st == XSwfBmpStatus::UnsupportedFormat) return SWFR_ERR_NOT_IMPLEMENTED;
        if (st != XSwfBmpStatus::Ok) return SWFR_ERR_INVALID;
        if (rgba) {
            if (rgba_cap < px.size()) return SWFR_ERR_CAPACITY;
            std::memcpy(rgba, px.data(), px.size());
        }
        return SWFR_OK;
    } catch (...) { return SWFR_ERR_DEVICE; }
}

int swfr_register_bitmap_tag(swfr_renderer* r, uint32_t id, const char* media_type, const uint8_t* data, size_t len) {
    if (!r || !media_type || !data) return fail(r, SWFR_ERR_INVALID, "null argument");
    if (std::strcmp(media_type, "image/x-swf-bmp") != 0)
        return fail(r, SWFR_ERR_NOT_IMPLEMENTED, std::string("NotImplemented: Support for ") + media_type + " images");   // node-canvas-bitmap-service.ts:34-35
    uint32_t w = 0, h = 0;
    std::vector<uint8_t> px;
    XSwfBmpStatus st = XSwfBmpStatus::Corrupt;
    try { st = decode_x_swf_bmp(data, len, w, h, px); } catch (...) { return fail(r, SWFR_ERR_DEVICE, "out of memory decoding a bitmap"); }
    if (st == XSwfBmpStatus::UnsupportedFormat) return fail(r, SWFR_ERR_NOT_IMPLEMENTED, std::string("UnsupportedXSwfBmpFormatId: ") + std::to_string(len ? int(data[0]) : -1));
    if (st != XSwfBmpStatus::Ok) return fail(r, SWFR_ERR_INVALID, "corrupt image/x-swf-bmp data");
    return swfr_register_bitmap(r, id, w, h, px.data(), size_t(w) * 4);
}

int swfr_register_bitmap(swfr_renderer* r, uint32_t id, uint32_t width, uint32_t height, const uint8_t* rgba, size_t stride) {
    if (!r || !rgba || width == 0 || height == 0 || stride < size_t(width) * 4) return fail(r, SWFR_ERR_INVALID, "bad bitmap");
    if (id > 65535) return fail(r, SWFR_ERR_INVALID, "bitmap id out of range");
    return guarded(r, [&]() {
        r->builder->add_bitmap(id, BitmapInfo{width, height});
        if (!r->has_device) return int(SWFR_OK);
        // putImageData: straight RGBA -> premultiplied ARGB (c * a / 255)
        std::vector<uint32_t> argb(size_t(width) * height);
        for (uint32_t y = 0; y < height; ++y) {
            const uint8_t* row = rgba + size_t(y) * stride;
            for (uint32_t x = 0; x < width; ++x) {
                const uint32_t a = row[4 * x + 3];
                const uint32_t pr = row[4 * x] * a / 255, pg = row[4 * x + 1] * a / 255, pb = row[4 * x + 2] * a / 255;
                argb[size_t(y) * width + x] = (a << 24) | (pr << 16) | (pg << 8) | pb;
            }
        }
        DeviceBitmap& slot = r->bitmaps[id];
        release_bitmap_slot(r, id, slot);
        slot.gen = ++r->bitmap_gen;                             // (the colour-transformed textures of the previous generation are stale)
        slot.straight.resize(size_t(width) * height * 4);
        for (uint32_t y = 0; y < height; ++y) std::memcpy(&slot.straight[size_t(y) * width * 4], rgba + size_t(y) * stride, size_t(width) * 4);
        HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&slot.pixels), argb.size() * 4));
        HIP_CHECK(hipMemcpy(slot.pixels, argb.data(), argb.size() * 4, hipMemcpyHostToDevice));
        slot.width = width;
        slot.height = height;
        if (r->bitmap_table.size() <= id) r->bitmap_table.resize(id + 1, DevBitmap{nullptr, 0, 0});
        r->bitmap_table[id] = DevBitmap{slot.pixels, width, height};
        r->bitmap_table_dirty = true;
        return int(SWFR_OK);
    });
}

int swfr_set_color_transform(swfr_renderer* r, uint32_t slot, const swfr_color_transform* ct) {
    if (!r) return SWFR_ERR_INVALID;
    if (slot > 65535) return fail(r, SWFR_ERR_INVALID, "colour transform slot out of range (0..65535)");
    if (ct && !color_transform_valid(*ct)) return fail(r, SWFR_ERR_INVALID, "colour transform value outside the int16 range");
    r->builder->set_color_transform(slot, ct);
    return SWFR_OK;
}

int swfr_set_shadow(swfr_renderer* r, uint32_t slot, const swfr_shadow* shadow) {
    if (!r) return SWFR_ERR_INVALID;
    if (slot > 65535) return fail(r, SWFR_ERR_INVALID, "shadow slot out of range (0..65535)");
    if (shadow && !shadow_valid(*shadow)) return fail(r, SWFR_ERR_INVALID, "InvalidShadow");
    r->builder->set_shadow(slot, shadow);
    return SWFR_OK;
}

int swfr_set_kernel(swfr_renderer* r, uint32_t slot, const swfr_kernel* kernel) {
    if (!r) return SWFR_ERR_INVALID;
    if (slot > 65535) return fail(r, SWFR_ERR_INVALID, "kernel slot out of range (0..65535)");
    if (kernel && !kernel_valid(*kernel)) return fail(r, SWFR_ERR_INVALID, "InvalidKernel");
    r->builder->set_kernel(slot, kernel);
    return SWFR_OK;
}

int swfr_set_filters(swfr_renderer* r, uint32_t slot, const swfr_filter* filters, uint32_t count) {
    if (!r) return SWFR_ERR_INVALID;
    if (slot > 65535) return fail(r, SWFR_ERR_INVALID, "InvalidFilter");
    if (filters && count > SWFR_MAX_FILTERS) return fail(r, SWFR_ERR_CAPACITY, "FilterListLength");
    for (uint32_t i = 0; filters && i < count; ++i)
        if (!filter_valid(filters[i])) return fail(r, SWFR_ERR_INVALID, "InvalidFilter");
    r->builder->set_filters(slot, filters, count);
    return SWFR_OK;
}

int swfr_debug_time_cxform(swfr_renderer* r, uint32_t bitmap_id, const swfr_color_transform* ct, uint32_t reps, float* pass_ms, float* copy_ms) {
    if (!r || !ct || !pass_ms || !copy_ms || reps == 0) return fail(r, SWFR_ERR_INVALID, "null argument");
    if (!r->has_device) return fail(r, SWFR_ERR_NO_DEVICE, "host-only handle cannot rasterize");
    if (!color_transform_valid(*ct)) return fail(r, SWFR_ERR_INVALID, "colour transform value outside the int16 range");
    return guarded(r, [&]() {
        const auto bit = r->bitmaps.find(bitmap_id);
        if (bit == r->bitmaps.end()) return fail(r, SWFR_ERR_NOT_FOUND, "BitmapNotFound");
        DeviceBitmap& bm = bit->second;
        const size_t n = size_t(bm.width) * bm.height, bytes = n * 4;
        cx_straight_on(bm, r->stream);
        uint32_t chain[256];
        for (int c = 0; c < 256; ++c) {
            uint32_t w = 0;
            for (int k = 0; k < 4; ++k) w |= uint32_t(std::clamp(((c * ct->mult[k]) >> 8) + ct->add[k], 0, 255)) << (8 * k);
            chain[c] = w;
        }
        uint32_t* out = nullptr;                                                                    // the texels, and behind them the table
        const auto pass = [&]() { launch_cxform_texels(r->stream, bm.d_straight, out, n, out + n); };
        const auto copy = [&]() { HIP_CHECK(hipMemcpyAsync(out, bm.d_straight, bytes, hipMemcpyDeviceToDevice, r->stream)); };
        return time_phases(r, reps, {{&out, bytes + CX_TABLE_BYTES, -1}}, [&]() {
            HIP_CHECK(hipMemcpyAsync(out + n, chain, CX_TABLE_BYTES, hipMemcpyHostToDevice, r->stream));
            HIP_CHECK(hipStreamSynchronize(r->stream));                                             // (`chain` is a local)
            pass(); copy();                                                                         // (warm-up)
        }, {{pass, pass_ms}, {copy, copy_ms}});
    });
}

int swfr_build_frame(swfr_renderer* r, const swfr_stage* stage, const swfr_edge** edges, size_t* n_edges, const swfr_path** paths,
                     size_t* n_paths, const swfr_style** styles, size_t* n_styles) {
    if (!r || !stage) return fail(r, SWFR_ERR_INVALID, "null argument");
    return guarded(r, [&]() {
        r->scene_from_builder = false;                          // (the builder's arrays are about to hold another frame than scene 0)
        r->builder->build(*stage);
        r->blur_table.clear();                                  // (the walk's blurred layers have no textures: only swfr_render makes them)
        if (edges) *edges = r->builder->edges().data();
        if (n_edges) *n_edges = r->builder->edges().size();
        if (paths) *paths = r->builder->paths().data();
        if (n_paths) *n_paths = r->builder->paths().size();
        if (styles) *styles = r->builder->styles().data();
        if (n_styles) *n_styles = r->builder->styles().size();
        return int(SWFR_OK);
    });
}

uint32_t swfr_built_layers(const swfr_renderer* r) { return r ? uint32_t(r->builder->layers().size()) : 0u; }

int swfr_built_layer(swfr_renderer* r, uint32_t k, const swfr_edge** edges, size_t* n_edges, const swfr_path** paths, size_t* n_paths,
                     const swfr_style** styles, size_t* n_styles, uint32_t* blur_x, uint32_t* blur_y, uint32_t* passes) {
    if (!r) return SWFR_ERR_INVALID;
    const auto& layers = r->builder->layers();
    if (k >= layers.size()) return fail(r, SWFR_ERR_NOT_FOUND, "no such blurred layer in the last built frame");
    const BlurLayer& B = layers[k];
    if (edges) *edges = B.edges.data();
    if (n_edges) *n_edges = B.edges.size();
    if (paths) *paths = B.paths.data();
    if (n_paths) *n_paths = B.paths.size();
    if (styles) *styles = B.styles.data();
    if (n_styles) *n_styles = B.styles.size();
    const bool conv = B.filters[0].kind == SWFR_FILTER_CONVOLUTION;      // (no box: its blur_x names a kernel slot)
    if (blur_x) *blur_x = conv ? 0u : B.filters[0].shadow.blur_x;
    if (blur_y) *blur_y = conv ? 0u : B.filters[0].shadow.blur_y;
    if (passes) *passes = conv ? 1u : B.filters[0].shadow.passes;
    return SWFR_OK;
}

int swfr_built_layer_shadow(swfr_renderer* r, uint32_t k, int* has_shadow, swfr_shadow* out) {
    if (!r) return SWFR_ERR_INVALID;
    const auto& layers = r->builder->layers();
    if (k >= layers.size()) return fail(r, SWFR_ERR_NOT_FOUND, "no such blurred layer in the last built frame");
    const bool shadowed = layers[k].type == SWFR_OBJECT_SHADOWED_LAYER;
    if (has_shadow) *has_shadow = shadowed ? 1 : 0;
    if (out && shadowed) *out = layers[k].filters[0].shadow;
    return SWFR_OK;
}

int swfr_built_layer_filters(swfr_renderer* r, uint32_t k, uint32_t* count, swfr_filter* out) {
    if (!r) return SWFR_ERR_INVALID;
    const auto& layers = r->builder->layers();
    if (k >= layers.size()) return fail(r, SWFR_ERR_NOT_FOUND, "no such blurred layer in the last built frame");
    if (count) *count = layers[k].n_filters;
    if (out) std::copy(layers[k].filters, layers[k].filters + layers[k].n_filters, out);
    return SWFR_OK;
}

int swfr_built_layer_kernel(swfr_renderer* r, uint32_t k, uint32_t entry, swfr_kernel* out) {
    if (!r) return SWFR_ERR_INVALID;
    const auto& layers = r->builder->layers();
    if (k >= layers.size()) return fail(r, SWFR_ERR_NOT_FOUND, "no such blurred layer in the last built frame");
    if (entry >= layers[k].n_filters || layers[k].filters[entry].kind != SWFR_FILTER_CONVOLUTION) return fail(r, SWFR_ERR_NOT_FOUND, "no such convolution entry in the layer's filter list");
    if (out) *out = layers[k].kernels[entry];
    return SWFR_OK;
}

int swfr_capture_bitmap(swfr_renderer* r, uint32_t bitmap_id) {
    if (!r) return SWFR_ERR_INVALID;
    if (bitmap_id > 65535) return fail(r, SWFR_ERR_INVALID, "bitmap id out of range");
    if (!r->has_device) return fail(r, SWFR_ERR_NO_DEVICE, "host-only handle has no image");
    if (r->cfg.band_count > 1) return fail(r, SWFR_ERR_NOT_IMPLEMENTED, "NotImplementedBlurBands");
    if (!r->fb_valid) return fail(r, SWFR_ERR_INVALID, "nothing rendered yet");
    return guarded(r, [&]() {
        wait_all_streams(r);
        const uint32_t* fb = r->fb_cur ? r->fb_cur : r->fs[0].d_fb.ptr;
        const size_t n = size_t(r->width) * r->height;
        DeviceBitmap& slot = r->bitmaps[bitmap_id];
        release_bitmap_slot(r, bitmap_id, slot);
        slot.gen = ++r->bitmap_gen;
        slot.captured = true;
        HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&slot.pixels), n * 4));
        slot.width = r->width; slot.height = r->height;
        launch_blur_capture(r->stream, fb, slot.pixels, n);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipStreamSynchronize(r->stream));
        BitmapInfo info{r->width, r->height};
        info.captured = true;
        r->builder->add_bitmap(bitmap_id, info);
        if (r->bitmap_table.size() <= bitmap_id) r->bitmap_table.resize(bitmap_id + 1, DevBitmap{nullptr, 0, 0});
        r->bitmap_table[bitmap_id] = DevBitmap{slot.pixels, slot.width, slot.height};
        r->bitmap_table_dirty = true;
        return int(SWFR_OK);
    });
}

int swfr_blur_bitmap(swfr_renderer* r, uint32_t bitmap_id, uint32_t blur_x, uint32_t blur_y, uint32_t passes) {
    if (!r) return SWFR_ERR_INVALID;
    if (blur_x > 255u || blur_y > 255u || passes == 0u || passes > 15u) return fail(r, SWFR_ERR_INVALID, "InvalidBlur");
    if (!r->has_device) return fail(r, SWFR_ERR_NO_DEVICE, "host-only handle has no bitmaps on a device");
    swfr_filter entry{};
    entry.kind = SWFR_FILTER_BLUR; entry.shadow.blur_x = blur_x; entry.shadow.blur_y = blur_y; entry.shadow.passes = passes;
    return filter_bitmap(r, bitmap_id, entry, nullptr);
}

int swfr_convolve_bitmap(swfr_renderer* r, uint32_t bitmap_id, const swfr_kernel* kernel) {
    if (!r) return SWFR_ERR_INVALID;
    if (!kernel || !kernel_valid(*kernel)) return fail(r, SWFR_ERR_INVALID, "InvalidKernel");
    if (!r->has_device) return fail(r, SWFR_ERR_NO_DEVICE, "host-only handle has no bitmaps on a device");
    swfr_filter entry{};
    entry.kind = SWFR_FILTER_CONVOLUTION;
    return filter_bitmap(r, bitmap_id, entry, kernel);
}

int swfr_shadow_bitmap(swfr_renderer* r, uint32_t dst_id, uint32_t src_id, const swfr_shadow* shadow) {
    if (!r) return SWFR_ERR_INVALID;
    if (!shadow || !shadow_valid(*shadow)) return fail(r, SWFR_ERR_INVALID, "InvalidShadow");
    if (dst_id > 65535) return fail(r, SWFR_ERR_INVALID, "bitmap id out of range");
    if (!r->has_device) return fail(r, SWFR_ERR_NO_DEVICE, "host-only handle has no bitmaps on a device");
    return guarded(r, [&]() {
        const auto sit = r->bitmaps.find(src_id);
        if (sit == r->bitmaps.end() || !sit->second.pixels) return fail(r, SWFR_ERR_NOT_FOUND, "BitmapNotFound");
        wait_all_streams(r);
        const uint32_t w = sit->second.width, h = sit->second.height;
        const size_t n = size_t(w) * h;
        // the alpha surface in one scratch texture, the box passes between the two, the finish pass into the destination's texels: a
        // new allocation, or the source's own -- the pass is pointwise
        r->shadow_scratch.reserve(n);
        if (blur_steps(shadow->blur_x, shadow->blur_y, shadow->passes)) r->blur_scratch.reserve(n);
        uint32_t* fresh = nullptr;
        if (dst_id != src_id) HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&fresh), std::max<size_t>(n, 1) * 4));
        const uint32_t* const group = sit->second.pixels;
        uint32_t* const out = fresh ? fresh : sit->second.pixels;
        launch_shadow_alpha(r->stream, group, r->shadow_scratch.ptr, w, h, shadow->dx, shadow->dy, (shadow->flags & SWFR_SHADOW_INNER) != 0u);
        const uint32_t* at = blur_image(r->stream, r->shadow_scratch.ptr, r->blur_scratch.ptr, w, h, shadow->blur_x, shadow->blur_y, shadow->passes);
        launch_shadow_finish(r->stream, at, group, false, out, n, shadow_color_pixel(shadow->color), shadow->strength, shadow->flags);
        const hipError_t launched = hipGetLastError(), done = hipStreamSynchronize(r->stream);
        if (launched != hipSuccess || done != hipSuccess) {
            if (fresh) (void)hipFree(fresh);
            HIP_CHECK(launched);
            HIP_CHECK(done);
        }
        bitmap_slot_has_new_texels(r, dst_id, out, w, h, false);     // (src_id's own slot and texels when the two are one)
        return int(SWFR_OK);
    });
}

// swfr_debug_time_shadow and swfr_debug_time_inner_shadow: the outer or the inner instances, the same buffers, the same order
static int time_shadow(swfr_renderer* r, bool inner, uint32_t width, uint32_t height, int32_t dx, int32_t dy, uint32_t reps, float* alpha_ms, float* finish_ms, float* copy_ms) {
    if (!r || !alpha_ms || !finish_ms || !copy_ms || reps == 0 || width == 0 || height == 0 || width > 32768 || height > 32768 || dx < -32768 ||
        dx > 32767 || dy < -32768 || dy > 32767)
        return fail(r, SWFR_ERR_INVALID, "bad argument");
    if (!r->has_device) return fail(r, SWFR_ERR_NO_DEVICE, "host-only handle cannot rasterize");
    return guarded(r, [&]() {
        const size_t n = size_t(width) * height, bytes = n * 4;
        uint32_t *a = nullptr, *b = nullptr, *c = nullptr;
        const uint32_t cp = 0x80402010u, flags = inner ? SWFR_SHADOW_INNER : 0u;
        const auto alpha = [&]() { launch_shadow_alpha(r->stream, a, b, width, height, dx, dy, inner); };
        // (in place over the alpha words, as swfr_render runs it: a result's alpha byte is the next repetition's input, whatever it is)
        const auto finish = [&]() { launch_shadow_finish(r->stream, b, c, true, b, n, cp, 1u, flags); };
        const auto copy = [&]() { HIP_CHECK(hipMemcpyAsync(b, a, bytes, hipMemcpyDeviceToDevice, r->stream)); };
        return time_phases(r, reps, {{&a, bytes, 0x5a}, {&b, bytes, -1}, {&c, bytes, 0x5a}}, [&]() {   // (warm-up of both kernels and the copy)
            alpha();
            launch_shadow_finish(r->stream, b, a, true, b, n, cp, 1u, flags);
            copy();
        }, {{alpha, alpha_ms}, {finish, finish_ms}, {copy, copy_ms}});
    });
}
int swfr_debug_time_shadow(swfr_renderer* r, uint32_t width, uint32_t height, int32_t dx, int32_t dy, uint32_t reps, float* alpha_ms, float* finish_ms, float* copy_ms) {
    return time_shadow(r, false, width, height, dx, dy, reps, alpha_ms, finish_ms, copy_ms);
}
int swfr_debug_time_inner_shadow(swfr_renderer* r, uint32_t width, uint32_t height, int32_t dx, int32_t dy, uint32_t reps, float* alpha_ms, float* finish_ms, float* copy_ms) {
    return time_shadow(r, true, width, height, dx, dy, reps, alpha_ms, finish_ms, copy_ms);
}

int swfr_debug_time_convolve(swfr_renderer* r, uint32_t width, uint32_t height, const swfr_kernel* kernel, uint32_t reps, float* fb_ms, float* tex_ms, float* capture_ms) {
    if (!r || !kernel || !kernel_valid(*kernel) || !fb_ms || !tex_ms || !capture_ms || reps == 0 || width == 0 || height == 0 || width > 32768 || height > 32768)
        return fail(r, SWFR_ERR_INVALID, "bad argument");
    if (!r->has_device) return fail(r, SWFR_ERR_NO_DEVICE, "host-only handle cannot rasterize");
    return guarded(r, [&]() {
        const size_t n = size_t(width) * height, bytes = n * 4;
        uint32_t *a = nullptr, *b = nullptr;
        const auto fb = [&]() { launch_convolve(r->stream, a, b, width, height, *kernel, true); };
        const auto tex = [&]() { launch_convolve(r->stream, a, b, width, height, *kernel, false); };
        const auto capture = [&]() { launch_blur_capture(r->stream, a, b, n); };     // the streaming roof: one read, one write of the same bytes
        return time_phases(r, reps, {{&a, bytes, 0x5a}, {&b, bytes, -1}}, [&]() { fb(); tex(); capture(); }, {{fb, fb_ms}, {tex, tex_ms}, {capture, capture_ms}});
    });
}

int swfr_debug_time_blur(swfr_renderer* r, uint32_t width, uint32_t height, uint32_t w, uint32_t reps, float* h_ms, float* v_ms, float* copy_ms) {
    if (!r || !h_ms || !v_ms || !copy_ms || reps == 0 || width == 0 || height == 0 || width > 32768 || height > 32768 || w < 2 || w > 255)
        return fail(r, SWFR_ERR_INVALID, "bad argument");
    if (!r->has_device) return fail(r, SWFR_ERR_NO_DEVICE, "host-only handle cannot rasterize");
    return guarded(r, [&]() {
        const size_t bytes = size_t(width) * height * 4;
        uint32_t *a = nullptr, *b = nullptr;
        const auto across = [&]() { launch_blur_pass(r->stream, a, b, width, height, w, false); };
        const auto down = [&]() { launch_blur_pass(r->stream, a, b, width, height, w, true); };
        const auto copy = [&]() { HIP_CHECK(hipMemcpyAsync(b, a, bytes, hipMemcpyDeviceToDevice, r->stream)); };
        return time_phases(r, reps, {{&a, bytes, 0x5a}, {&b, bytes, -1}}, [&]() { across(); down(); copy(); },   // (warm-up of both kernels and the copy)
                           {{across, h_ms}, {down, v_ms}, {copy, copy_ms}});
    });
}

int swfr_upload_edges(swfr_renderer* r, const swfr_edge* edges, size_t n_edges, const swfr_path* paths, size_t n_paths,
                      const swfr_style* styles, size_t n_styles) {
    if (!r || (n_edges && !edges) || (n_paths && !paths) || (n_styles && !styles)) return fail(r, SWFR_ERR_INVALID, "null argument");
    ++r->cx_epoch;
    return guarded(r, [&]() {
        const SceneView sv{edges, n_edges, paths, n_paths, styles, n_styles};
        validate_upload(r, sv);
        return upload2(r, 0, true, sv, nullptr, false);
    });
}

int swfr_render_resident(swfr_renderer* r, uint32_t frames) {
    if (!r) return SWFR_ERR_INVALID;
    return guarded(r, [&]() { return render_resident(r, frames); });
}

int swfr_render_edges(swfr_renderer* r, const swfr_edge* edges, size_t n_edges, const swfr_path* paths, size_t n_paths,
                      const swfr_style* styles, size_t n_styles) {
    const int rc = swfr_upload_edges(r, edges, n_edges, paths, n_paths, styles, n_styles);
    if (rc != SWFR_OK) return rc;
    return swfr_render_resident(r, 1);
}

int swfr_render(swfr_renderer* r, const swfr_stage* stage) { return render_stage(r, stage, true); }

int swfr_last_path_timing(swfr_renderer* r, swfr_path_timing* out) {
    if (!r || !out) return SWFR_ERR_INVALID;
    *out = r->path_timing;
    return SWFR_OK;
}

int swfr_render_sequence(swfr_renderer* r, const swfr_stage* stages, uint32_t n_stages, uint32_t repeat, double* seconds, swfr_path_timing* sum) {
    if (!r || (!stages && n_stages) || !seconds) return fail(r, SWFR_ERR_INVALID, "null argument");
    swfr_path_timing acc{};
    const auto t0 = std::chrono::steady_clock::now();
    for (uint32_t rep = 0; rep < repeat; ++rep)
        for (uint32_t i = 0; i < n_stages; ++i) {
            const int rc = render_stage(r, &stages[i], false);
            if (rc != SWFR_OK) return rc;
            const swfr_path_timing& pt = r->path_timing;
            acc.build_ms += pt.build_ms; acc.upload_host_ms += pt.upload_host_ms; acc.h2d_ms += pt.h2d_ms; acc.device_ms += pt.device_ms;
            acc.total_ms += pt.total_ms; acc.h2d_bytes += pt.h2d_bytes;
        }
    *seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (sum) *sum = acc;
    return SWFR_OK;
}

// render + get_image per frame, the loop of the reference's own tests (HeadlessGfxRenderer::get_image after every render,
// rs/src/headless_renderer.rs:233-244): the mapped read-back of every frame, waited for at once (overlap == 0) or after the NEXT
// frame's swfr_render has returned -- its copy then overlaps that frame's host build (overlap != 0).  *checksum: the sum of one
// pixel per frame, so that every frame's image has been looked at.
int swfr_render_sequence_readback(swfr_renderer* r, const swfr_stage* stages, uint32_t n_stages, uint32_t repeat, int premultiplied, int overlap,
                                  double* seconds, uint64_t* checksum) {
    if (!r || (!stages && n_stages) || !seconds) return fail(r, SWFR_ERR_INVALID, "null argument");
    const auto t0 = std::chrono::steady_clock::now();
    uint64_t sum = 0;
    bool pending = false;
    const uint8_t* data = nullptr;
    const size_t mid = (size_t(r->height / 2) * r->width + r->width / 2) * 4;
    for (uint32_t rep = 0; rep < repeat; ++rep)
        for (uint32_t i = 0; i < n_stages; ++i) {
            int rc = render_stage(r, &stages[i], false);
            if (rc != SWFR_OK) return rc;
            if (pending) { rc = swfr_read_image_wait(r, &data, nullptr); if (rc != SWFR_OK) return rc; sum += data[mid] + data[mid + 3]; pending = false; }
            rc = swfr_read_image_async(r, premultiplied);
            if (rc != SWFR_OK) return rc;
            pending = true;
            if (!overlap) { rc = swfr_read_image_wait(r, &data, nullptr); if (rc != SWFR_OK) return rc; sum += data[mid] + data[mid + 3]; pending = false; }
        }
    if (pending) { const int rc = swfr_read_image_wait(r, &data, nullptr); if (rc != SWFR_OK) return rc; sum += data[mid] + data[mid + 3]; }
    *seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (checksum) *checksum = sum;
    return SWFR_OK;
}

int swfr_render_batch(swfr_renderer* r, const swfr_stage* stages, uint32_t n_stages, void* device_dst, size_t frame_stride) {
    if (!r || (!stages && n_stages)) return fail(r, SWFR_ERR_INVALID, "null argument");
    if (!r->has_device) return fail(r, SWFR_ERR_NO_DEVICE, "host-only handle cannot rasterize");
    if (device_dst && !(word_aligned(device_dst) && word_aligned(frame_stride))) return fail(r, SWFR_ERR_INVALID, "MisalignedTarget");
    ++r->cx_epoch;
    return guarded(r, [&]() { return render_batch(r, stages, n_stages, device_dst, frame_stride); });
}

int swfr_read_image(swfr_renderer* r, uint8_t* dst, size_t dst_stride, int premultiplied) {
    if (!r || !dst || dst_stride < size_t(r->width) * 4) return fail(r, SWFR_ERR_INVALID, "bad destination");
    if (!r->has_device) return fail(r, SWFR_ERR_NO_DEVICE, "host-only handle has no image");
    if (!r->fb_valid) return fail(r, SWFR_ERR_INVALID, "nothing rendered yet");
    return guarded(r, [&]() {
        const size_t n = size_t(r->width) * r->height;
        const uint32_t* src = r->fb_cur ? r->fb_cur : r->fs[0].d_fb.ptr;
        if (!premultiplied) {
            r->d_tmp.reserve(n);
            launch_unpremultiply(r->stream, src, r->d_tmp.ptr, n);
            src = r->d_tmp.ptr;
        }
        HIP_CHECK(hipMemcpy2DAsync(dst, dst_stride, src, size_t(r->width) * 4, size_t(r->width) * 4, r->height, hipMemcpyDeviceToHost,
                                   r->stream));
        HIP_CHECK(hipStreamSynchronize(r->stream));
        return int(SWFR_OK);
    });
}

int swfr_read_image_async(swfr_renderer* r, int premultiplied) {
    if (!r) return SWFR_ERR_INVALID;
    if (!r->has_device) return fail(r, SWFR_ERR_NO_DEVICE, "host-only handle has no image");
    if (!r->fb_valid) return fail(r, SWFR_ERR_INVALID, "nothing rendered yet");
    return guarded(r, [&]() { return start_read(r, premultiplied); });
}

int swfr_read_image_wait(swfr_renderer* r, const uint8_t** data, size_t* stride) {
    if (!r || !data) return fail(r, SWFR_ERR_INVALID, "null argument");
    if (!r->has_device) return fail(r, SWFR_ERR_NO_DEVICE, "host-only handle has no image");
    return guarded(r, [&]() {
        const int rc = finish_read(r);
        if (rc == SWFR_OK) { *data = r->h_image; if (stride) *stride = size_t(r->width) * 4; }
        return rc;
    });
}

int swfr_render_resident_batched(swfr_renderer* r, uint32_t frames_per_launch, uint32_t launches, float* total_ms) {
    if (!r) return SWFR_ERR_INVALID;
    return guarded(r, [&]() { return render_resident_batched(r, frames_per_launch, launches, total_ms); });
}

int swfr_shape_json(swfr_renderer* r, uint32_t id, int morph, const char** json) {
    if (!r || !json) return fail(r, SWFR_ERR_INVALID, "null argument");
    return guarded(r, [&]() {
        const DecodedShape* s = r->builder->shape(id, morph != 0);
        if (!s) throw StatusError{SWFR_ERR_NOT_FOUND, "unknown shape id"};
        r->json_scratch = shape_to_json(*s);
        *json = r->json_scratch.c_str();
        return int(SWFR_OK);
    });
}

int swfr_last_timing(swfr_renderer* r, swfr_timing* out) {
    if (!r || !out) return SWFR_ERR_INVALID;
    *out = r->timing;
    return SWFR_OK;
}

size_t swfr_band_slab_bytes(const swfr_renderer* r) {
    if (!r) return 0;
    const BandShare bs = band_share(r);
    return size_t(bs.stride == 1 && r->cfg.band_count > 1 ? bs.padded : bs.count) * TILE_H * r->width * 4;    // (contiguous blocks: every rank's slab has the common size)
}

int swfr_copy_band_slab(swfr_renderer* r, void* device_dst) {
    if (!r || !device_dst) return fail(r, SWFR_ERR_INVALID, "null argument");
    if (!r->has_device) return fail(r, SWFR_ERR_NO_DEVICE, "host-only handle");
    return guarded(r, [&]() {
        const BandShare bs = band_share(r);
        if (bs.stride == 1 && r->cfg.band_count > 1) {         // one contiguous block of rows: a plain copy, zero padding behind it
            const uint32_t* fb = r->fb_cur ? r->fb_cur : r->fs[0].d_fb.ptr;
            const size_t row_bytes = size_t(r->width) * 4, y0 = size_t(bs.first) * TILE_H;
            const size_t rows = y0 >= r->height ? 0 : std::min<size_t>(size_t(bs.count) * TILE_H, r->height - y0);
            if (rows) HIP_CHECK(hipMemcpyAsync(device_dst, reinterpret_cast<const uint8_t*>(fb) + y0 * row_bytes, rows * row_bytes, hipMemcpyDeviceToDevice, r->stream));
            const size_t total = size_t(bs.padded) * TILE_H;
            if (total > rows) HIP_CHECK(hipMemsetAsync(static_cast<uint8_t*>(device_dst) + rows * row_bytes, 0, (total - rows) * row_bytes, r->stream));
            HIP_CHECK(hipStreamSynchronize(r->stream));
            return int(SWFR_OK);
        }
        const uint32_t bc = r->cfg.band_count > 1 ? r->cfg.band_count : 1, bi = r->cfg.band_count > 1 ? r->cfg.band_index : 0;
        launch_pack_band(r->stream, r->fb_cur ? r->fb_cur : r->fs[0].d_fb.ptr, static_cast<uint32_t*>(device_dst), int(r->width), int(r->height), bi, bc, local_tile_rows(r));
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipStreamSynchronize(r->stream));
        return int(SWFR_OK);
    });
}

int swfr_set_targets(swfr_renderer* r, void* const* device_targets, uint32_t n_targets) {
    if (!r || n_targets > 4 || (n_targets && !device_targets)) return fail(r, SWFR_ERR_INVALID, "bad targets");
    for (uint32_t k = 0; k < n_targets; ++k)                  // (refused as a whole: the handle keeps the targets it had)
        if (!word_aligned(device_targets[k])) return fail(r, SWFR_ERR_INVALID, "MisalignedTarget");
    r->n_targets = n_targets;
    for (uint32_t k = 0; k < n_targets; ++k) r->targets[k] = static_cast<uint32_t*>(device_targets[k]);
    r->scene_ready = false;                               // the frame descriptors carry the framebuffer address: upload again
    return SWFR_OK;
}

int swfr_render_resident_async(swfr_renderer* r, uint32_t* out_set) {
    return r ? render_resident_async(r, nullptr, out_set) : SWFR_ERR_INVALID;
}

int swfr_render_resident_async_to(swfr_renderer* r, void* block_target, uint32_t* out_set) {
    if (!r || !block_target) return SWFR_ERR_INVALID;
    if (!word_aligned(block_target)) return fail(r, SWFR_ERR_INVALID, "MisalignedTarget");
    return render_resident_async(r, block_target, out_set);
}

int swfr_render_resident_group_to(swfr_renderer* r, void* const* block_targets, uint32_t n_frames, uint32_t* sets_used) {
    if (!r || !block_targets || n_frames == 0 || n_frames > 64) return SWFR_ERR_INVALID;
    for (uint32_t i = 0; i < n_frames; ++i)                  // (before the first launch: no frame of the group is queued)
        if (block_targets[i] && !word_aligned(block_targets[i])) return fail(r, SWFR_ERR_INVALID, "MisalignedTarget");
    uint32_t used = 0;
    for (uint32_t i = 0; i < n_frames; ++i) {
        uint32_t k = 0;
        const int rc = swfr_render_resident_async_to(r, block_targets[i], &k);
        if (rc != SWFR_OK) return rc;
        used |= 1u << k;
    }
    if (sets_used) *sets_used = used;
    return SWFR_OK;
}

int swfr_get_stats(swfr_renderer* r, swfr_stats* out) {
    if (!r || !out) return SWFR_ERR_INVALID;
    *out = r->stats;
    return SWFR_OK;
}

void* swfr_stream_handle(swfr_renderer* r, uint32_t set) { return (r && r->has_device && set < 4) ? static_cast<void*>(r->fs[set].stream) : nullptr; }

int swfr_wait(swfr_renderer* r) {
    if (!r) return SWFR_ERR_INVALID;
    if (!r->has_device) return fail(r, SWFR_ERR_NO_DEVICE, "host-only handle");
    return guarded(r, [&]() {
        uint32_t* const host = pinned_counters(r);
        int rc = SWFR_OK;
        for (uint32_t k = 0; k < 4; ++k) {
            if (!r->fs[k].stream || !r->fs[k].counters) continue;
            if (r->async_used >> k & 1u) queue_counters(r->fs[k].stream, host + k * COUNTER_WORDS, r->fs[k].counters);
            HIP_CHECK(hipStreamSynchronize(r->fs[k].stream));
            if (r->async_used >> k & 1u) rc = check_frames(r, host + k * COUNTER_WORDS, 1, rc);
        }
        r->async_used = 0;
        r->fb_valid = rc == SWFR_OK;
        return rc;
    });
}

long swfr_debug_copy(swfr_renderer* r, int what, void* dst, size_t bytes) {
    if (!r || !dst) return -long(SWFR_ERR_INVALID);
    if (!r->has_device) return -long(SWFR_ERR_NO_DEVICE);
    if (what == 2 || what == 3) {      // (no device buffer: what the last launch chain chose; the row launches of the last resident call that binned the next frame)
        if (bytes < sizeof(uint32_t)) return 0;
        std::memcpy(dst, what == 2 ? &r->last_bin_threads : &r->last_ahead_launches, sizeof(uint32_t));
        return long(sizeof(uint32_t));
    }
    if (!r->fs[0].work.ptr) return 0;
    // frame set 0's descriptor as upload2 carved it (scene slot 0's sizes), and the bytes its row headers and cells take
    const FrameDims& d = r->scn[0].dims;
    Frame2 f{};
    carve_frame(f, d, r->fs[0].work.ptr);
    const void* src = what == 0 ? static_cast<const void*>(f.rows) : static_cast<const void*>(f.cells);
    const size_t n = std::min(bytes, what == 0 ? d.row_count() * sizeof(RowInfo2) : d.cell_count() * sizeof(Cell));
    if (!n) return 0;
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(dst, src, n, hipMemcpyDeviceToHost) != hipSuccess) return -long(SWFR_ERR_DEVICE);
    return long(n);
}

void* swfr_device_framebuffer(swfr_renderer* r) { return (r && r->has_device) ? (r->fb_cur ? r->fb_cur : r->fs[0].d_fb.ptr) : nullptr; }

#pragma GCC visibility pop
}  // extern "C"
