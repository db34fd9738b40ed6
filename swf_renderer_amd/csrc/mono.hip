// mono.hip -- the aliased row pass (SWFR_FLAG_ANTIALIAS_NONE; included by raster2.hip, not a translation unit of its own).
//
// Cairo 1.16 under CAIRO_ANTIALIAS_NONE converts a non-rectilinear polygon at pixel CENTRES (cairo-mono-scan-converter.c; the
// bounded operators' _cairo_rasterise_polygon_to_boxes has the same arithmetic).  With I(v) = (v + 127) >> 8 (24.8 -> pixel, ties
// down):
//   * an edge is active in pixel row y when I(top) <= y < I(bottom) (inside the converter's rows);
//   * its crossing there is x = x1 + floor((256 y + 127 - y1) (x2 - x1) / (y2 - y1)) -- at the row's centre less 1/256 (CAIRO_FIXED_ONE / 2
//     - 1: probed against libcairo 1.16.0, 7 297 of 7 297 rows of random slanted edges; at 256 y + 128 seven of them differ), stepped
//     from row to row with a floored quotient and remainder, which is this exact quotient every row -- at pixel I(x);
//   * the row's crossings are walked in x order with the winding: a span opens where the winding leaves zero and closes where it comes
//     back to zero, unless the next crossing's pixel is at most one further -- so a ONE-pixel gap between two spans is filled;
//   * a span [xs, xe) is clipped to the converter's columns [x_min, x_max).
// Only the PIXEL order of the crossings matters: inside a group of crossings at one pixel the winding may pass through zero, but the
// next crossing is then at the same pixel and nothing closes; the group decides only through the winding before and after it.  So a
// group g (pixel p_g) opens a span iff the winding before it is zero and p_g > p_{g-1} + 1 (or g is the first), and closes one iff
// the winding after it is zero and p_{g+1} > p_g + 1 (or g is the last) -- a local rule, no edge-list history, no tie replay.
//
// Output: what k2_rows writes for a tor path -- row headers, cells (a span is make_cell(xs - x_min, 15, 0), make_cell(xe - x_min, -15, 0)),
// class bytes, StripTop notes and strip costs -- so k2_tiles paints the spans at full coverage without knowing the mode.
//   k2_rows_mono       one wavefront per row chunk (the chunk records of k2_bin), lane = pixel row: the chunk's edges are read as the
//                      raw records (wave-uniform, scalar loads), each lane keeps its row's crossings as sorted keys (pixel, direction)
//                      in MONO_NS registers (insertion by min / max), walks them with the rule above and writes its cells itself --
//                      at most one per active edge, so the chunk's fixed region (17 cells per incidence) always holds them.
//   k2_rows_mono_huge  a row with more than MONO_NS crossings: one 1024-thread workgroup, the crossings binned per pixel column in LDS
//                      (count and winding per column; left of the columns one bin, the column x_max one bin), a workgroup prefix sum of
//                      the winding, the rule above per column, cells through the bump allocator.  Up to 8 192 active edges per row as
//                      in the antialiased path; more -> E2_ACTIVE_EDGES (SWFR_ERR_CAPACITY).

#define MONO_NS 16                      // crossings per row the chunk kernel keeps in registers
#define MONO_BIAS (1 << 17)             // pixels of crossings lie within +-(2^15 + 1): biased keys are positive
#define MONO_INVALID 0xffffffffu        // sorts behind every key; its pixel is far right of every real one
#define MONO_BIN_PT 9                   // pixel-column bins per thread of k2_rows_mono_huge: 8 192 columns + 2
#define MONO_BINS (MONO_BIN_PT * HUGE_THREADS)

__device__ __forceinline__ int mono_round(int v) { return (v + 127) >> 8; }          // _cairo_fixed_integer_round_down
// the pixel rows [ra, rb) an edge is active in, inside the converter's rows
__device__ __forceinline__ void mono_rows(const swfr_edge& e, const DevPath& P, int& ra, int& rb) {
    ra = max(mono_round(e.top), P.y_min);
    rb = e.top < e.bottom ? min(mono_round(e.bottom), P.y_max) : ra;
}
// the pixel of an active edge's crossing with pixel row y (1/256 above its centre, as Cairo): the exact floor quotient, estimated with the reciprocal and
// fixed up with the exact remainder (|numerator| < 2^48: every f64 value here is an integer held exactly)
__device__ __forceinline__ int mono_pixel(const swfr_edge& e, int y) {
    const int dx = e.x2 - e.x1;
    if (dx == 0) return mono_round(e.x1);
    const double dy = (double)(e.y2 - e.y1);
    const double num = (double)(256 * y + 127 - e.y1) * (double)dx;
    double q = floor(num * (1.0 / dy));
    const double rem = fma(-q, dy, num);
    if (rem < 0.0) q -= 1.0;
    else if (rem >= dy) q += 1.0;
    return mono_round(e.x1 + (int)q);
}
__device__ __forceinline__ uint32_t mono_key(int px, int dir) { return ((uint32_t)(px + MONO_BIAS) << 1) | (dir > 0 ? 1u : 0u); }
__device__ __forceinline__ int mono_key_px(uint32_t k) { return (int)(k >> 1) - MONO_BIAS; }
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) v = max(v, __shfl_xor(v, o));
    return v;
}

__device__ __forceinline__ void mono_chunk_body(FramePtr FR, uint32_t block) {
    const int lane = threadIdx.x;
    const ChunkInfo ck = FR->chunks[block];                               // wave-uniform: path and edge reads are scalar
    const uint32_t lo = ck.path;
    const DevPath P = FR->paths[lo];
    const swfr_edge* __restrict__ E = FR->raw + ck.first_edge;
    const int r = (int)ck.first_row + lane;
    const int chunk_rows = (int)ck.rows;
    // the band entry of this lane's tile-row: where its row header and class bytes go (as k2_rows)
    const int g16 = (((int)ck.first_row & (TILE_H - 1)) + lane) >> 4;
    const int band = (int)ck.first_row / TILE_H + g16;
    const int band_lo = P.y_min / TILE_H, band_hi = (P.y_max - 1) / TILE_H;
    BandSlot cls_bs = {0u, 0u, 0u, 0u};
    uint32_t cls_b0 = 0, cls_b1 = 0;
    if (ck.slot0 != ~0u && lane < chunk_rows) {
        cls_bs = FR->band_slots[ck.slot0 + (uint32_t)g16];
        const uint32_t bclamp = min((uint32_t)band, FR->n_bands - 1u);
        cls_b0 = FR->band_off[bclamp];
        cls_b1 = FR->band_off[bclamp + 1u];
    }
    const bool band_ok = ck.slot0 != ~0u && lane < chunk_rows && band >= band_lo && band <= band_hi && P.kind == SWFR_PATH_TOR;
    const uint32_t ri = band_ok ? cls_bs.slot * TILE_H + (uint32_t)(r & (TILE_H - 1)) : ~0u;
    const bool in_path = P.kind == SWFR_PATH_TOR && lane < chunk_rows && r >= P.y_min && r < P.y_max;
    bool live = in_path;
    { uint32_t lb; if (live && !owns_band(FR, r / TILE_H, lb)) live = false; }         // another rank's tile-row
    if (__ballot(live) == 0ull) {
        if (ri != ~0u) { RowInfo2 h; h.off = 0; h.n = 0; h.mode = (uint16_t)(in_path ? (uint32_t)ROW_FOREIGN : (uint32_t)ROW_EMPTY); FR->rows[ri] = h; }
        return;
    }
    const int row0 = (int)ck.first_row, row1 = row0 + chunk_rows;
    // ---- (edge, pixel row) pairs of this path above the chunk: where its cells start (lanes = edges)
    int inc_before = 0;
    for (uint32_t eb = 0; eb < ck.n_edges; eb += 64) {
        const uint32_t k = eb + (uint32_t)lane;
        if (k < ck.n_edges) {
            int ra, rb;
            mono_rows(E[k], P, ra, rb);
            inc_before += max(0, min(rb, row0) - ra);
        }
    }
    const uint32_t chunk_cell_base = ck.rec_base * (uint32_t)MAX_CELLS_PER_EDGE_ROW + (uint32_t)__builtin_amdgcn_readlane(wave_scan_incl(inc_before), 63);
    // ---- the row's crossings as sorted keys: one insertion (min / max down the slots) per active edge
    uint32_t key[MONO_NS];
#pragma unroll
    for (int s = 0; s < MONO_NS; ++s) key[s] = MONO_INVALID;
    int n = 0, nmax = 0;                                                 // nmax: wave-uniform bound on the keys any lane holds
    for (uint32_t k = 0; k < ck.n_edges; ++k) {                          // (wave-uniform: scalar loads)
        const swfr_edge e = E[k];
        int ra, rb;
        mono_rows(e, P, ra, rb);
        if (rb <= max(ra, row0) || ra >= row1) continue;                  // not active in the chunk's rows
        const bool act = live && r >= ra && r < rb;
        uint32_t kk = act ? mono_key(mono_pixel(e, r), e.dir) : MONO_INVALID;
        n += act ? 1 : 0;
        nmax = min(nmax + 1, MONO_NS);
#pragma unroll
        for (int s = 0; s < MONO_NS; ++s) {
            if (s >= nmax) break;                                        // wave-uniform
            const uint32_t a = key[s];
            key[s] = min(a, kk);
            kk = max(a, kk);
        }
        if (__ballot(live && n <= MONO_NS) == 0ull) break;               // every row goes to the general routine anyway
    }
    const bool over = live && n > MONO_NS;
    nmax = wave_max(over ? 0 : min(n, MONO_NS));
    const unsigned fmask = P.fill_rule ? 1u : ~0u;
    // ---- room: at most one cell per crossing (a span has two ends, each at a crossing)
    const int room = live && !over && ri != ~0u ? n : 0;
    const uint32_t incl_cells = (uint32_t)wave_scan_incl(room);
    const uint32_t total_cells = (uint32_t)__builtin_amdgcn_readlane((int)incl_cells, 63);
    const uint32_t wave_base = ((uint64_t)chunk_cell_base + total_cells <= (uint64_t)FR->cell_slice) ? chunk_cell_base : ~0u;
    if (wave_base == ~0u && lane == 0) atomicOr(&FR->counters[C2_ERROR], E2_CELL_ARENA);
    const uint32_t my_room = wave_base + incl_cells - (uint32_t)room;
    // ---- the walk: cells, and over the first 32 tile columns of the path's rectangle the columns with a cell / covered right of them
    const int tc0 = P.x_min / TILE_W, tc1 = (P.x_max - 1) / TILE_W, ntc = tc1 - tc0 + 1;
    int n_cells = 0;
    uint32_t m_inter = 0, m_cov = 0;
    if (room > 0 && wave_base != ~0u) {
        Cell* __restrict__ dst = FR->cells + my_room;
        int w = 0, xs = 0;
#pragma unroll
        for (int p = 0; p < MONO_NS; ++p) {
            if (p >= nmax) break;                                        // wave-uniform
            const uint32_t kp = key[p];
            if (kp == MONO_INVALID) continue;
            const int x = mono_key_px(kp);
            const int xp = p > 0 ? mono_key_px(key[p - 1]) : -(1 << 30);
            const int xn = p + 1 < MONO_NS ? mono_key_px(key[p + 1]) : (1 << 30);
            const int wb = w;
            w += (kp & 1u) ? 1 : -1;
            if (((unsigned)wb & fmask) == 0u && x > xp + 1) xs = x;       // a group that opens a span (x > xp + 1: first of its group, not adjacent)
            if (((unsigned)w & fmask) == 0u && xn > x + 1) {              // a group that closes it (xn > x + 1: last of its group, next one not adjacent)
                const int a = max(xs, P.x_min), b = min(x, P.x_max);
                if (b > a) {
                    dst[n_cells++] = make_cell(a - P.x_min, 15, 0);
                    const int ta = a / TILE_W - tc0;
                    m_inter |= col_bit(ta); m_cov ^= cols_from(ta + 1);
                    if (b < P.x_max) {
                        dst[n_cells++] = make_cell(b - P.x_min, -15, 0);
                        const int tb = b / TILE_W - tc0;
                        m_inter |= col_bit(tb); m_cov ^= cols_from(tb + 1);
                    }
                }
            }
        }
    }
    const uint32_t mode = n_cells ? (uint32_t)ROW_FULL : (uint32_t)ROW_EMPTY;
    // ---- row headers (a row left to k2_rows_mono_huge gets its header there)
    if (ri != ~0u) {
        RowInfo2 h; h.off = 0; h.n = 0;
        h.mode = (uint16_t)(over ? (uint32_t)ROW_DEFER : (in_path && !live) ? (uint32_t)ROW_FOREIGN : mode);
        if (n_cells) { h.off = my_room; h.n = (uint16_t)n_cells; }
        FR->rows[ri] = h;
    }
    // ---- rows left to k2_rows_mono_huge (counted as queued and as crowded rows)
    {
        const bool q = over && ri != ~0u;
        const unsigned long long qm = __ballot(q);
        if (qm) {
            uint32_t qbase = 0;
            if (lane == 0) {
                qbase = atomicAdd(&FR->counters[C2_HUGE], (uint32_t)__popcll(qm));
                atomicAdd(&FR->counters[C2_SLOW], (uint32_t)__popcll(qm));
            }
            qbase = (uint32_t)__builtin_amdgcn_readfirstlane((int)qbase);
            if (q) {
                const uint32_t at = qbase + (uint32_t)__popcll(qm & ((1ull << lane) - 1ull));
                if (at < FR->slow_cap) { SlowRow sr; sr.path = lo; sr.row = r; sr.ri = ri; sr.pad = 0; FR->huge[at] = sr; }
                else atomicOr(&FR->counters[C2_ERROR], E2_SLOW_QUEUE);
            }
        }
    }
    // ---- class bytes of the chunk's (strip, tile column) pairs from the rows' masks, as k2_rows: lanes 8j .. 8j + 7 are the rows of
    //      the chunk's j-th strip; a row is full or empty in every tile column without a cell (m_cov tells which)
    if (ck.slot0 != ~0u && P.kind == SWFR_PATH_TOR) {
        const int width = FR->width, height = FR->height;
        uint8_t* out = FR->cls;
        uint32_t n_b = 0;
        if (band_ok) {
            n_b = cls_b1 - cls_b0;
            out = FR->cls + (size_t)STRIPS_PER_TILE * FR->tiles_x * cls_b0 + (cls_bs.slot - cls_b0);
        }
        const swfr_style& st = style_at(FR, P.style);
        const uint32_t opq = (st.kind == SWFR_STYLE_SOLID && P.lerp && (st.pixel >> 24) == 0xffu) ? CLS_OPAQUE : 0u;
        const bool in_frame = r < height && band_ok, in_rows = in_frame && in_path;
        uint32_t local_trow = 0;
        const bool own_band = band_ok && owns_band(FR, band, local_trow);
        const bool cost_order = FR->strip_order != 0u;
        const uint32_t pos1 = cls_bs.slot - cls_b0 + 1u;
        const int strip_in_tile = (r >> 3) & 1, tsub = lane & 7;
        for (int tb = 0; tb < ntc; tb += 32) {                           // wave-uniform
            const int nb = min(ntc - tb, 32);
            const uint32_t colmask = nb >= 32 ? ~0u : ((1u << nb) - 1u);
            // beyond the first 32 tile columns a row with cells counts as partial everywhere
            uint32_t iv = tb == 0 ? m_inter : (n_cells ? ~0u : 0u), cv = tb == 0 ? m_cov : 0u;
            uint32_t inside = colmask;
            if (tb == 0 && P.x_min > tc0 * TILE_W) inside &= ~1u;
            if (tb + nb == ntc && P.x_max < min((tc1 + 1) * TILE_W, width)) inside &= ~(1u << (nb - 1));
            uint32_t mp = 0, mn = 0, me = 0, mh = 0;
            if (in_frame) {
                if (!in_rows) mn = colmask;
                else if (over) { mp = mn = me = colmask; }               // decided by k2_rows_mono_huge: the general route is always right
                else {
                    iv &= colmask; cv &= colmask;
                    mp = iv | (cv & ~inside);
                    me = iv | cv;
                    mh = colmask & ~me;
                    mn = mp | mh;
                }
            }
            const unsigned long long pb = __ballot(in_rows && (over || (iv & colmask) != 0u));
#define MONO_OR8(v) do { v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xf, 0xf, false); \
                         v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xb1, 0xf, 0xf, false); \
                         v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4e, 0xf, 0xf, false); } while (0)
            MONO_OR8(mp); MONO_OR8(mn); MONO_OR8(me); MONO_OR8(mh);
#undef MONO_OR8
            mp |= mh & me;                                               // rows without coverage beside rows with: partial
            for (int t0 = 0; t0 < nb; t0 += 8) {                         // wave-uniform
                const int t = t0 + tsub;
                uint32_t f = (((mp >> t) & 1u) ? CLS_PARTIAL : 0u) | (((mn >> t) & 1u) ? CLS_NOTFULL : 0u) | (((me >> t) & 1u) ? CLS_NONEMPTY : 0u);
                if (f == CLS_NONEMPTY) f |= opq;
                const int tc = tc0 + tb + t;
                if (t < nb && band_ok && lane < chunk_rows) {
                    out[(uint32_t)(tc * STRIPS_PER_TILE + strip_in_tile) * n_b] = (uint8_t)f;
                    if (own_band) {
                        const uint32_t strip_id = (local_trow * (uint32_t)FR->tiles_x + (uint32_t)tc) * STRIPS_PER_TILE + (uint32_t)strip_in_tile;
                        strip_top_note(FR, strip_id, pos1, f, st.pixel);
                        if (cost_order && (f & CLS_PARTIAL)) {
                            const uint32_t wgt = (uint32_t)__popcll((pb >> (lane & ~7)) & 0xffull);
                            if (wgt) atomicAdd(&FR->strip_cost[strip_id], wgt);
                        }
                    }
                }
            }
        }
    }
}

// workgroup-wide exclusive prefix sum of one value per thread (HUGE_THREADS threads); *total = the sum
__device__ __forceinline__ int mono_block_scan(int v, int* total) {
    __shared__ int wave_tot[HUGE_THREADS / 64];
    const int tid = threadIdx.x, wave = tid >> 6;
    const int incl = wave_scan_incl(v);
    if ((tid & 63) == 63) wave_tot[wave] = incl;
    __syncthreads();
    int before = 0, all = 0;
    for (int k = 0; k < HUGE_THREADS / 64; ++k) { const int t = wave_tot[k]; if (k < wave) before += t; all += t; }
    __syncthreads();                                                     // (wave_tot is rewritten by the next scan)
    *total = all;
    return before + incl - v;
}

// one queued row: bins per pixel column hold crossings << 16 + winding (|winding| <= crossings <= 8 192); bin 0 = everything left of
// x_min (only its winding matters: a span open there starts at x_min, one closed there is clipped away), bin W + 1 = the column x_max
// (only whether a crossing is there: it keeps a span open to the right edge); crossings right of x_max change nothing
__device__ __forceinline__ void mono_huge_row(FramePtr FR, const SlowRow sr) {
    __shared__ int bins[MONO_BINS];
    __shared__ uint32_t n_active, cell_base;
    const int tid = threadIdx.x;
    const DevPath P = FR->paths[sr.path];
    const int y = sr.row, W = P.x_max - P.x_min, nbins = W + 2;
    for (int b = tid; b < nbins; b += HUGE_THREADS) bins[b] = 0;
    if (tid == 0) n_active = 0;
    __syncthreads();
    uint32_t mine = 0;
    for (uint32_t k = (uint32_t)tid; k < P.n_edges; k += HUGE_THREADS) {
        const swfr_edge e = FR->raw[P.first_edge + k];
        int ra, rb;
        mono_rows(e, P, ra, rb);
        if (y < ra || y >= rb) continue;
        ++mine;
        const int px = mono_pixel(e, y);
        if (px > P.x_max) continue;
        atomicAdd(&bins[px < P.x_min ? 0 : px - P.x_min + 1], 65536 + (e.dir > 0 ? 1 : -1));
    }
    if (mine) atomicAdd(&n_active, mine);
    __syncthreads();
    if (n_active > (uint32_t)ROWS_HUGE_MAXA) {                           // (workgroup-uniform) the antialiased path's capacity: refused
        if (tid == 0) {
            atomicOr(&FR->counters[C2_ERROR], E2_ACTIVE_EDGES);
            RowInfo2 h; h.off = 0; h.n = 0; h.mode = (uint16_t)ROW_EMPTY; FR->rows[sr.ri] = h;
        }
        return;
    }
    const unsigned fmask = P.fill_rule ? 1u : ~0u;
    auto crossings = [&](int b) { return b < nbins ? (bins[b] + 32768) >> 16 : 0; };
    // this thread's bins [b0, b0 + MONO_BIN_PT): the winding entering them, then the rule per column
    const int b0 = tid * MONO_BIN_PT;
    int sum = 0;
#pragma unroll
    for (int j = 0; j < MONO_BIN_PT; ++j) { const int b = b0 + j; if (b < nbins) { const int v = bins[b]; sum += v - crossings(b) * 65536; } }
    int dummy;
    int w = mono_block_scan(sum, &dummy);
    uint32_t starts = 0, ends = 0;                                       // bit j: a span starts / ends at the column of bin b0 + j
#pragma unroll
    for (int j = 0; j < MONO_BIN_PT; ++j) {
        const int b = b0 + j;
        if (b >= nbins) break;
        const int c = crossings(b), wb = w;
        w += bins[b] - c * 65536;
        if (b == 0 || b == nbins - 1) continue;
        const bool has = c > 0, z_before = ((unsigned)wb & fmask) == 0u, z_after = ((unsigned)w & fmask) == 0u;
        const bool start = b == 1 ? (has || !z_before) : (has && z_before && crossings(b - 1) == 0);
        const bool end = has && z_after && crossings(b + 1) == 0;
        if (start && !end) starts |= 1u << j;
        if (end && !start) ends |= 1u << j;
    }
    int total = 0;
    const int cnt = __popc(starts | ends);
    const int before = mono_block_scan(cnt, &total);
    if (tid == 0) {
        uint32_t base = 0;
        if (total) {
            const uint32_t old = atomicAdd(&FR->counters[C2_HEAD], (uint32_t)total);
            base = FR->cell_main + old;
            if ((uint64_t)base + (uint32_t)total > FR->cell_slice) { atomicOr(&FR->counters[C2_ERROR], E2_CELL_ARENA); base = ~0u; }
        }
        cell_base = base;
    }
    __syncthreads();
    const uint32_t base = cell_base;
    if (base != ~0u) {
        Cell* dst = FR->cells + base + before;
        for (uint32_t m = starts | ends; m; m &= m - 1u) {
            const int j = __ffs((int)m) - 1;
            *dst++ = make_cell(b0 + j - 1, ((starts >> j) & 1u) ? 15 : -15, 0);
        }
    }
    if (tid == 0) {
        RowInfo2 h; h.off = base == ~0u ? 0u : base; h.n = base == ~0u ? (uint16_t)0 : (uint16_t)total;
        h.mode = (uint16_t)(total ? ROW_FULL : ROW_EMPTY);
        FR->rows[sr.ri] = h;
    }
}
__device__ __forceinline__ void mono_huge_loop(FramePtr FR) {
    const uint32_t n_rows = min(FR->counters[C2_HUGE], FR->slow_cap);
    for (uint32_t i = blockIdx.x; i < n_rows; i += gridDim.x) {
        mono_huge_row(FR, FR->huge[i]);
        __syncthreads();
    }
}
