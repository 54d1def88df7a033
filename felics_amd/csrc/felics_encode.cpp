// felics_encode.cpp -- encoding frames of one shape: what a lane queues for a sub-batch (8-bit: run_lane, 16-bit: run_wide), the
// outcome of a sub-batch and the remedies, the blocking call (encode_device), the submission queue and the host-buffer path.
//
// Encode is GPU-only by design: there is no CPU encode path in this library.
#include "felics_host.h"
#include "felics_index.h"

namespace felics {

namespace {

// Everything one sub-batch of 8-bit frames needs, queued without waiting for the host (tile-local layout, felics_kernels.h):
//   front stream : one fill that clears the sub-batch's counters, sums and chain states; then slice by slice the front kernel
//                  (classify + sort a tile's events, once) and the records of the slice's chains (k_enum)
//   spine stream : behind every k_enum the spine launch that walks the slice's chains
//   k stream     : behind every spine launch the k of the slice's events (k_assign3); a context of four lanes has no k stream
//                  and queues them on the front stream, behind the NEXT slice's two launches
//   tail stream  : behind every k launch -- when every stream has a fixed slot in the output -- the packed bits of that
//                  slice's tiles (k_pack_t: code lengths, tile offsets by look-back, packing in one kernel); RGB planes 1, 2
//                  go to scratch slots and are moved behind plane 0 at the end (the offset of planes 1 and 2 needs the size
//                  of the planes before them).
// The stream sizes are copied to the lane's pinned buffer and `sized` is recorded behind them.
// slot_stride == 0: no packing here (the caller places the streams exactly once it has the sizes).
template <typename T, typename ET>
int run_lane(felics_ctx *ctx, Lane &l, uint8_t *d_out, uint64_t slot_stride) {
    const Geometry &g = l.g;
    const int ns = l.nslices;
    const size_t nsamples = (size_t)g.nplanes * g.npix;
    int rc = 0;
    // Fixed slots: code lengths, tile offsets and packing in one kernel per slice (k_pack_t; one such kernel at a time unless the
    // tiles are handed out by ticket: the tiles of two of them waiting for each other's queued predecessors could hold all
    // workgroup slots, so the lanes share the tail stream).  Otherwise (exact placement, FELICS_TWO_PASS, after a look-back gave
    // up twice): k to a byte per pixel once every chain is replayed, then the lengths / bit scan / pack kernels over all tiles.
    const bool fused = (slot_stride != 0 || g.mixed != nullptr) && !ctx->two_pass;  // (a mixed sub-batch: slots from its table, never two-pass)
    const uint32_t cap = ctx->cap_max ? tile_cap_max(g.nctx, g.npix) : ctx->test_tile_cap ? std::min(4u * REC, tile_cap_max(g.nctx, g.npix)) : tile_cap_default(g.nctx, g.npix);
    const size_t ptiles = (size_t)g.nplanes * g.sort_tiles;
    const size_t slots = ptiles * cap, recs = slots / REC;
    const size_t nchains = (size_t)g.nplanes * g.nctx;
    if ((rc = reserve(ctx, l.evs, slots * sizeof(ET) + STAGE_PAD)) != 0) return rc;
    if ((rc = reserve(ctx, l.pix_of, slots * 2 + STAGE_PAD)) != 0) return rc;
    if ((rc = reserve(ctx, l.k_sorted, slots + STAGE_PAD)) != 0) return rc;
    if ((rc = reserve(ctx, l.counts, ptiles * g.nctx * 4)) != 0) return rc;        // the run table
    if ((rc = reserve(ctx, l.tile_slots, ptiles * 4)) != 0) return rc;
    if ((rc = reserve(ctx, l.desc, recs * 8 + 64)) != 0) return rc;
    if ((rc = reserve(ctx, l.block_state, recs * 16 + 64)) != 0) return rc;         // state16
    if ((rc = reserve(ctx, l.partial, (size_t)SLICES * nchains * 8)) != 0) return rc;  // chain_seg per slice
    if (!fused && (rc = reserve(ctx, l.k_map, nsamples + STAGE_PAD)) != 0) return rc;
    if (!fused && (rc = reserve(ctx, l.group_bits, (size_t)g.nplanes * g.pack_tiles * PACK_THREADS * 2)) != 0) return rc;
    if ((rc = reserve(ctx, l.tile_bits, (size_t)g.nplanes * g.pack_tiles * 4)) != 0) return rc;
    if ((rc = reserve(ctx, l.tile_bitoff, (size_t)g.nplanes * g.pack_tiles * 8)) != 0) return rc;
    // The cleared block: everything a sub-batch wants zero when it starts, in one allocation, so that ONE fill at the head of the
    // front stream clears it (the lane is idle then: its last sub-batch's sizes have been waited for) and ONE copy brings the
    // sizes, the error word and the flags back:
    //   image_bytes[nimages] | d_error, d_flags | d_tickets[SLICES + 2], d_nrec[SLICES] | carry[nplanes], base[nplanes] | chain_state
    const size_t o_words = (size_t)g.nimages * 8, o_counters = o_words + 8;
    const size_t o_sums = (o_counters + 4 * (2 * SLICES + 2) + 15) & ~(size_t)15;
    const size_t o_chain = (o_sums + (size_t)g.nplanes * 16 + 255) & ~(size_t)255;
    const size_t cleared = o_chain + nchains * 32;
    if ((rc = reserve(ctx, l.image_bytes, cleared)) != 0) return rc;
    if ((rc = reserve(ctx, l.image_off, (size_t)(g.nimages + 1) * 8)) != 0) return rc;
    if ((rc = reserve_zeroed(ctx, l.status, (size_t)g.nplanes * g.pack_tiles * 8)) != 0) return rc;
    if ((rc = reserve(ctx, l.edge_first, (size_t)g.nplanes * g.pack_tiles * 4)) != 0) return rc;
    if ((rc = reserve(ctx, l.edge_last, (size_t)g.nplanes * g.pack_tiles * 4)) != 0) return rc;
    const size_t hs = (size_t)g.nimages * 2 + 1;
    if ((rc = reserve_pinned(ctx, (void **)&l.h_sizes, l.h_sizes_cap, hs, hs * 8 + 64)) != 0) return rc;
    hipStream_t s = l.stream, f = l.front, tl = l.tail;
    // k_assign3 of slice q follows spine[q] and goes in front of pack[q]: on the lane's k stream, or -- four lanes: the low pool is
    // full of front streams -- on the front stream behind enum[q + 1], which does not wait for the spine
    hipStream_t ks = ctx->assign_on == ASSIGN_TAIL ? tl : l.kstream ? l.kstream : f;
    if (ctx->serial) f = ks = tl = s;  // FELICS_SERIAL (profiling: every kernel alone): one stream, same order of launches
    const T *d_planes = (const T *)l.d_planes;
    uint8_t *block = (uint8_t *)l.image_bytes.p;
    auto *chain_state = (uint32_t *)(block + o_chain);
    auto *plane_carry = (uint64_t *)(block + o_sums);
    auto *plane_base = plane_carry + g.nplanes;
    l.plane_base = plane_base;
    const EpochStep tag = lookback_epoch_next(l.epoch);  // look-back tags: 18 epoch bits, cleared in front of the front kernel when they wrap (felics_epochs.h)
    if (tag.clear) HIP_TRY(ctx, hipMemsetAsync(l.status.p, 0, l.status.cap, f));
    const uint32_t epoch = l.epoch = tag.epoch;
    if (ctx->trace_epochs) fprintf(stderr, "[felics] look-back lane %d epoch 0x%x clear %d\n", (int)(&l - ctx->lanes), epoch, (int)tag.clear);
    PackTarget target{d_out, slot_stride, nullptr, 0};
    if (fused && g.planes_per_image > 1) {
        target.plane_slot = ((uint64_t)g.npix + g.npix / 4 + 64 + 15) & ~15ull;
        if ((rc = reserve(ctx, l.pscratch, (size_t)(target.plane_slot * g.nimages * (g.planes_per_image - 1)))) != 0) return rc;
        target.scratch = (uint8_t *)l.pscratch.p;
    }
    uint32_t *d_error = (uint32_t *)(block + o_words);  // look-back watchdog of the single-pass pack
    uint32_t *d_flags = d_error + 1;  // TL_FLAG_*: the front kernel's order check and tile overflow, the spine's self-check (read back together with d_error)
    uint32_t *d_tickets = (uint32_t *)(block + o_counters);  // one per pack launch of this sub-batch: tiles are handed out in order
    uint32_t *d_nrec = d_tickets + SLICES + 2;  // records per slice
    const TileLocal<ET> tloc{(ET *)l.evs.p, (uint16_t *)l.pix_of.p, (uint8_t *)l.k_sorted.p, (uint32_t *)l.counts.p, (uint32_t *)l.tile_slots.p, cap};
    l.m_tickets = ctx->pack_tickets;
    l.m_fused = fused;
    l.m_cap = cap;

    uint32_t bounds[SLICES + 1];  // slice boundaries in sort tiles (= pack tiles)
    for (int q = 0; q <= ns; q++) bounds[q] = (uint32_t)((uint64_t)g.sort_tiles * q / ns);
    // the records of slice q live in their own region of desc: as many as its tiles can hold
    auto slice_of = [&](int q) {
        const size_t r0 = (size_t)bounds[q] * g.nplanes * (cap / REC);
        return ChainSlice{(uint2 *)l.desc.p + r0, (uint2 *)l.partial.p + (size_t)q * nchains, d_nrec + q, (uint4 *)l.block_state.p};
    };
    // ---- front stream
    if (ctx->poison) {  // FELICS_POISON: every intermediate buffer starts as garbage, as on a fresh context
        DevBuf *bufs[] = {&l.evs, &l.pix_of, &l.k_sorted, &l.counts, &l.tile_slots, &l.desc, &l.block_state, &l.partial, &l.k_map,
                          &l.group_bits, &l.tile_bits, &l.tile_bitoff, &l.edge_first, &l.edge_last, &l.pscratch};
        for (DevBuf *b : bufs)
            if (b->p) HIP_TRY(ctx, hipMemsetAsync(b->p, 0xA5, b->cap, f));
    }
    HIP_TRY(ctx, hipMemsetAsync(block, 0, cleared, f));  // (the tail's words too: every tail launch follows an assign launch, and that this fill)
    // (FELICS_TEST_SCATTER_ORDER: the atomically ranked kernel reports a violation whatever it produced; the ballot-ranked form is
    // the remedy and is checked for real)
    const uint32_t front_mode = ctx->scatter_ballot ? FRONT_SAFE_RANK : ctx->test_scatter_order ? FRONT_TEST_VIOLATION : 0u;
    if (!ctx->scatter_ballot) ctx->stats.sorted_event_sorts++;
    // behind every spine launch, k of the slice's events and -- when every stream has a fixed slot -- the packed bits of the slice's
    // tiles on the tail stream.  Queued one slice late, so that on the front stream the k launch stands behind the NEXT slice's
    // front and enum launches (which do not wait for the spine) and not in front of them.
    auto behind_spine = [&](int q) -> int {
        HIP_TRY(ctx, hipStreamWaitEvent(ks, l.spine_done[q], 0));
        if (bounds[q + 1] != bounds[q]) {
            StageTimer t(ctx, l, ST_ASSIGN, ks, true);
            launch_assign3<ET>(ks, tloc, (const uint4 *)l.block_state.p, g, bounds[q], bounds[q + 1]);
        }
        HIP_TRY(ctx, hipEventRecord(l.assign_done[q], ks));
        if (!fused) return FELICS_OK;
        HIP_TRY(ctx, hipStreamWaitEvent(tl, l.assign_done[q], 0));
        if (bounds[q + 1] == bounds[q]) return FELICS_OK;
        StageTimer t(ctx, l, ST_PACK, tl, true);
        launch_pack_t<T>(tl, d_planes, tloc.kq, tloc.pix, tloc.ev, tloc.tile_slots, cap, (uint64_t *)l.status.p, (uint64_t *)l.tile_bitoff.p,
                         (uint32_t *)l.tile_bits.p, plane_carry, (uint32_t *)l.edge_first.p, (uint32_t *)l.edge_last.p, d_error, target, g,
                         bounds[q], bounds[q + 1], epoch, ctx->pack_tickets ? d_tickets + q : nullptr);
        return FELICS_OK;
    };
    for (int q = 0; q < ns; q++) {
        if (bounds[q + 1] != bounds[q]) {
            {
                StageTimer t(ctx, l, ST_SCATTER, f, true);
                launch_front<T, ET>(f, d_planes, tloc, g, bounds[q], bounds[q + 1], d_flags, front_mode);
            }
            // the slice's records in chain order: here, not on the spine stream, so that it runs beside the previous slice's walk
            StageTimer t(ctx, l, ST_OFFSETS, f, true);
            launch_enum(f, tloc.runtab, slice_of(q), g, bounds[q], bounds[q + 1], cap);
        }
        HIP_TRY(ctx, hipEventRecord(l.slice_done[q], f));
        // ---- spine stream: the walk along every chain
        HIP_TRY(ctx, hipStreamWaitEvent(s, l.slice_done[q], 0));
        if (bounds[q + 1] != bounds[q]) {
            StageTimer t(ctx, l, ST_SPINE, s, true);
            launch_spine3<ET>(s, tloc.ev, slice_of(q), chain_state, d_flags, g);
        }
        HIP_TRY(ctx, hipEventRecord(l.spine_done[q], s));
        if (q > 0 && (rc = behind_spine(q - 1)) != 0) return rc;
    }
    if ((rc = behind_spine(ns - 1)) != 0) return rc;
    // ---- tail stream: the sizes, and the streams' last touches
    if (fused) {
        StageTimer t(ctx, l, ST_ZERO, tl);
        launch_finish_sizes(tl, plane_carry, plane_base, (uint64_t *)l.image_bytes.p, g);
        launch_join_edges(tl, (const uint64_t *)l.tile_bitoff.p, (const uint32_t *)l.tile_bits.p,
                          (const uint32_t *)l.edge_first.p, (const uint32_t *)l.edge_last.p, target, g);
        launch_concat_planes(tl, plane_base, plane_carry, target, g);
        if (l.idx_rows) {
            // A mixed sub-batch whose images want restart indexes: here, behind the pack, join and concat of every tile and in front
            // of the copy of the sizes, so that `sized` -- what the host waits for before it reuses the lane or returns -- stands
            // behind the indexes too.  Written whatever the sub-batch's flags will say: one that is redone gets them again.
            for (const auto &z : l.idx_zero) HIP_TRY(ctx, hipMemsetAsync(z.first, 0, z.second, tl));
            launch_index_emit_mixed(tl, tloc.runtab, (const uint4 *)l.block_state.p, cap, (const uint64_t *)l.tile_bitoff.p, plane_base, plane_carry, g,
                                    l.idx_rows, l.idx_max_K);
        }
    } else {
        HIP_TRY(ctx, hipStreamWaitEvent(tl, l.assign_done[ns - 1], 0));
        {
            StageTimer t(ctx, l, ST_ASSIGN, tl, true);
            launch_k_to_pixels_tl(tl, tloc.kq, tloc.pix, tloc.tile_slots, cap, (uint8_t *)l.k_map.p, g);
        }
        {
            StageTimer t(ctx, l, ST_LENGTHS, tl, true);
            launch_lengths<T>(tl, d_planes, (const uint8_t *)l.k_map.p, (uint16_t *)l.group_bits.p,
                              (uint32_t *)l.tile_bits.p, g, 0, g.pack_tiles);
        }
        {
            StageTimer t(ctx, l, ST_BITSCAN, tl);
            launch_bitscan_slice(tl, (const uint32_t *)l.tile_bits.p, (uint64_t *)l.tile_bitoff.p, plane_carry, g, 0, g.pack_tiles);
            launch_finish_sizes(tl, plane_carry, plane_base, (uint64_t *)l.image_bytes.p, g);
        }
        if (slot_stride != 0) {
            {
                StageTimer t(ctx, l, ST_ZERO, tl);
                launch_zero_edges(tl, d_out, nullptr, slot_stride, (const uint64_t *)l.tile_bitoff.p,
                                  (const uint32_t *)l.tile_bits.p, plane_base, g, 0, g.pack_tiles);
            }
            StageTimer t(ctx, l, ST_PACK, tl, true);
            launch_pack<T>(tl, d_planes, (const uint8_t *)l.k_map.p, (const uint16_t *)l.group_bits.p,
                           (const uint64_t *)l.tile_bitoff.p, (const uint32_t *)l.tile_bits.p, plane_base, nullptr,
                           slot_stride, d_out, g, 0, g.pack_tiles);
        }
    }
    HIP_TRY(ctx, hipGetLastError());
    l.h_sizes[g.nimages] = 0;
    HIP_TRY(ctx, hipMemcpyAsync(l.h_sizes, block, o_counters, hipMemcpyDeviceToHost, tl));  // the sizes, then d_error | d_flags << 32
    HIP_TRY(ctx, hipEventRecord(l.sized, tl));
    if (ctx->profiling) HIP_TRY(ctx, hipEventRecord(l.span_end, tl));
    return FELICS_OK;
}

// 16-bit samples (T = u16 gray planes, i32 Y/Co/Cg planes): everything on the lane's main stream.
//   keys -> stable sort by (plane, context) -> chain heads -> estimator replay per chain (k_map)
//   -> lengths, bit scan, sizes -> pack (fixed slots) ; same contract as run_lane towards the caller.
template <typename T>
int run_wide(felics_ctx *ctx, Lane &l, uint8_t *d_out, uint64_t slot_stride) {
    const Geometry &g = l.g;
    const size_t nsamples = (size_t)g.nplanes * g.npix;
    const WideSizes z = wide_sizes(g);
    int rc;
    for (int i = 0; i < 2; i++)
        if ((rc = reserve(ctx, l.wrecs[i], z.rec_bytes)) != 0) return rc;
    if ((rc = reserve(ctx, l.wtile_cnt, z.tile_cnt_bytes)) != 0) return rc;
    if ((rc = reserve(ctx, l.wmeta, z.meta_bytes)) != 0) return rc;
    if ((rc = reserve(ctx, l.whist, z.hist_bytes)) != 0) return rc;
    if ((rc = reserve(ctx, l.wdigtot, z.digtot_bytes)) != 0) return rc;
    if ((rc = reserve(ctx, l.heads, z.heads_bytes)) != 0) return rc;
    if ((rc = reserve(ctx, l.scalars, 64)) != 0) return rc;
    uint32_t lane_limit = wide_lane_limit(g);
    if (const char *e = getenv("FELICS_WIDE_LANE")) lane_limit = (uint32_t)std::max(0, atoi(e));  // tests, A/B: 0 = wave-wide only
    const size_t nlong = wide_long_capacity(g, lane_limit);
    if ((rc = reserve(ctx, l.wlong, nlong * (8 + 64) + 64)) != 0) return rc;
    if ((rc = reserve(ctx, l.k_map, nsamples + STAGE_PAD)) != 0) return rc;
    if ((rc = reserve(ctx, l.group_bits, (size_t)g.nplanes * g.pack_tiles * PACK_THREADS * sizeof(group_bits_t<T>))) != 0) return rc;
    if ((rc = reserve(ctx, l.tile_bits, (size_t)g.nplanes * g.pack_tiles * 4)) != 0) return rc;
    if ((rc = reserve(ctx, l.tile_bitoff, (size_t)g.nplanes * g.pack_tiles * 8)) != 0) return rc;
    if ((rc = reserve(ctx, l.plane_sums, (size_t)g.nplanes * 16)) != 0) return rc;
    if ((rc = reserve(ctx, l.image_bytes, (size_t)g.nimages * 8)) != 0) return rc;
    if ((rc = reserve(ctx, l.image_off, (size_t)(g.nimages + 1) * 8)) != 0) return rc;
    const size_t hs = (size_t)g.nimages * 2 + 1;
    if ((rc = reserve_pinned(ctx, (void **)&l.h_sizes, l.h_sizes_cap, hs, hs * 8 + 64)) != 0) return rc;
    hipStream_t s = l.stream;
    const T *d_planes = (const T *)l.d_planes;
    auto *plane_carry = (uint64_t *)l.plane_sums.p;
    auto *plane_base = plane_carry + g.nplanes;
    l.plane_base = plane_base;
    auto *nheads = (uint32_t *)l.scalars.p;
    if (ctx->poison) {
        DevBuf *bufs[] = {&l.wrecs[0], &l.wrecs[1], &l.wtile_cnt, &l.wmeta, &l.whist, &l.heads, &l.k_map,
                          &l.group_bits, &l.tile_bits, &l.tile_bitoff};
        for (DevBuf *b : bufs) HIP_TRY(ctx, hipMemsetAsync(b->p, 0xA5, b->cap, s));
    }
    {
        StageTimer t(ctx, l, ST_WIDE_KEYS, s);
        launch_wide_events<T>(s, d_planes, (uint32_t *)l.wtile_cnt.p, (uint32_t *)l.wmeta.p, (uint64_t *)l.wrecs[0].p, g);
    }
    {
        StageTimer t(ctx, l, ST_WIDE_SORT, s);
        launch_wide_sort(s, (uint64_t *)l.wrecs[0].p, (uint64_t *)l.wrecs[1].p, (const uint32_t *)l.wmeta.p, (uint32_t *)l.whist.p,
                         (uint32_t *)l.wdigtot.p, g);
    }
    {
        StageTimer t(ctx, l, ST_WIDE_CHAINS, s);
        HIP_TRY(ctx, hipMemsetAsync(nheads, 0, 8, s));
        launch_wide_chains(s, (const uint64_t *)l.wrecs[0].p, (const uint32_t *)l.wmeta.p, (uint64_t *)l.heads.p, nheads,
                           (uint8_t *)l.k_map.p, g, lane_limit, (uint64_t *)l.wlong.p, (uint32_t *)((uint64_t *)l.wlong.p + nlong));
    }
    HIP_TRY(ctx, hipMemsetAsync(plane_carry, 0, (size_t)g.nplanes * 16, s));
    {
        StageTimer t(ctx, l, ST_LENGTHS, s, true);
        launch_lengths<T>(s, d_planes, (const uint8_t *)l.k_map.p, (group_bits_t<T> *)l.group_bits.p,
                          (uint32_t *)l.tile_bits.p, g, 0, g.pack_tiles);
    }
    {
        StageTimer t(ctx, l, ST_BITSCAN, s);
        launch_bitscan_slice(s, (const uint32_t *)l.tile_bits.p, (uint64_t *)l.tile_bitoff.p, plane_carry, g, 0,
                             g.pack_tiles);
        launch_finish_sizes(s, plane_carry, plane_base, (uint64_t *)l.image_bytes.p, g);
    }
    if (slot_stride != 0 || g.mixed) {  // (a mixed sub-batch: every stream into the slot its table row names)
        {
            StageTimer t(ctx, l, ST_ZERO, s);
            launch_zero_edges(s, d_out, nullptr, slot_stride, (const uint64_t *)l.tile_bitoff.p,
                              (const uint32_t *)l.tile_bits.p, plane_base, g, 0, g.pack_tiles);
        }
        {
            StageTimer t(ctx, l, ST_PACK, s, true);
            launch_pack<T>(s, d_planes, (const uint8_t *)l.k_map.p, (const group_bits_t<T> *)l.group_bits.p,
                           (const uint64_t *)l.tile_bitoff.p, (const uint32_t *)l.tile_bits.p, plane_base, nullptr,
                           slot_stride, d_out, g, 0, g.pack_tiles);
        }
    }
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(l.h_sizes, l.image_bytes.p, (size_t)g.nimages * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipEventRecord(l.sized, s));
    if (ctx->profiling) HIP_TRY(ctx, hipEventRecord(l.span_end, s));
    return FELICS_OK;
}

// Exact placement: streams back to back at image_off (computed on the device from the sizes), every
// byte of them zeroed, all tiles packed.  Used when the streams do not get fixed slots, and to redo a
// sub-batch in which a stream outgrew its slot.
template <typename T>
int pack_exact(felics_ctx *ctx, Lane &l, uint8_t *d_out) {
    const Geometry &g = l.g;
    hipStream_t s = l.tail;
    const uint64_t *plane_base = l.plane_base;
    {
        StageTimer t(ctx, l, ST_ZERO, s);
        launch_zero_streams(s, (uint32_t *)d_out, (const uint64_t *)l.image_off.p, g);
    }
    {
        StageTimer t(ctx, l, ST_PACK, s, true);
        launch_pack<T>(s, (const T *)l.d_planes, (const uint8_t *)l.k_map.p, (const group_bits_t<T> *)l.group_bits.p,
                       (const uint64_t *)l.tile_bitoff.p, (const uint32_t *)l.tile_bits.p, plane_base,
                       (const uint64_t *)l.image_off.p, 0, d_out, g, 0, g.pack_tiles);
    }
    HIP_TRY(ctx, hipGetLastError());
    return FELICS_OK;
}

}  // namespace

// images per pass so that slots / chain bases (8-bit) or sample indices and sort keys (16-bit) stay below 2^32
size_t max_images_per_pass(uint64_t npix, uint32_t planes, int depth) {
    const uint64_t per_image = npix * planes;
    if (per_image == 0) return SIZE_MAX;
    if (const char *e = getenv("FELICS_TEST_PASS_IMAGES"))  // tests: several passes without a 100 GB batch
        return (size_t)std::max(1, atoi(e));
    if (depth == FELICS_DEPTH_16) {
        // ~30 bytes of workspace per sample: keep a pass near 2^30 samples -- and near 2^16 planes: the 16-bit front end scans
        // tiles x planes counts in one workgroup and searches the plane table per sort tile (a batch of many tiny frames)
        constexpr uint64_t WIDE_MAX_PLANES = 1u << 16;
        return (size_t)std::max<uint64_t>(1, std::min<uint64_t>(0x40000000ull / per_image, WIDE_MAX_PLANES / planes));
    }
    // the records of a pass are numbered with 32 bits: tiles x records per tile (worst case)
    const uint64_t tiles = (npix + SORT_TILE - 1) / SORT_TILE;
    const uint64_t rec_per_image = tiles * planes * (tile_cap_max(NCTX, (uint32_t)std::min<uint64_t>(npix, SORT_TILE)) / REC);
    // ... and a pass carries at most PASS_MAX_CHAINS = 2^23 chains (plane x context: 2^15 gray planes, 5 461 RGB images -- a batch
    // of many tiny frames).  partial / chain_prog hold SLICES * 8 + 32 bytes per chain, so the per-chain workspace of a pass stops
    // at 2^23 * 128 B = 1 GiB per lane (200 000 gray 8 x 8 frames as one pass held 9 GB), and felics_chain.hip numbers chains
    // (plane * nctx + ctx) and sizes k_enum's and k_spine3's grids by them in 32 bits.  Not 2^24: k_enum runs one 256-thread
    // workgroup per chain (planes rounded up to eight), and a grid of exactly 2^24 of them -- 2^32 work-items, a full pass of
    // 2^16 gray planes -- is refused by the runtime ("invalid configuration argument")
    const uint64_t chains_per_image = (uint64_t)planes * (planes == 3 ? nctx_of<int16_t>() : nctx_of<uint8_t>());
    return (size_t)std::max<uint64_t>(
        1, std::min<uint64_t>({0xE0000000ull / per_image, 0xE0000000ull / rec_per_image, PASS_MAX_CHAINS / chains_per_image}));
}

// What every launcher of a sub-batch does first: the lane's slices, the counters, the profiling pairs, and the geometry of `cnt`
// images whose planes are w x h samples (a mixed sub-batch: the padded planes; its launcher sets g.mixed / g.pitched afterwards).
Geometry &begin_sub_batch(felics_ctx *ctx, Lane &l, size_t first, size_t cnt, uint32_t w, uint32_t h, int color, int depth, int nslices, bool queued) {
    l.nslices = std::max(1, std::min(nslices, SLICES));
    l.queued = queued;
    l.first_image = first;
    l.idx_rows = nullptr;
    l.idx_max_K = 0;
    l.idx_zero.clear();
    ctx->stats.submissions++;
    for (int i = 0; i < ST_COUNT; i++) l.ev_used[i] = 0;
    const uint32_t planes = color == FELICS_COLOR_RGB ? 3 : 1;
    const uint64_t npix = (uint64_t)w * h;
    Geometry &g = l.g;
    g.mixed = nullptr;
    g.pitched = nullptr;
    g.pitched16 = nullptr;
    g.W = w;
    g.H = h;
    g.npix = (uint32_t)npix;
    g.nimages = (uint32_t)cnt;
    g.planes_per_image = planes;
    g.nplanes = (uint32_t)(cnt * planes);
    g.sort_tiles = (uint32_t)((npix + SORT_TILE - 1) / SORT_TILE);
    g.pack_tiles = (uint32_t)((npix + PACK_TILE - 1) / PACK_TILE);
    g.color = (uint32_t)color;
    g.depth = (uint32_t)depth;
    g.nctx = planes == 3 ? nctx_of<int16_t>() : nctx_of<uint8_t>();  // (16-bit samples: run_wide has tables of its own)
    return g;
}

// Everything the lane's geometry asks for behind the colour planes: run_lane (8-bit) or run_wide (16-bit) on the lane's sample type.
int run_sub_batch(felics_ctx *ctx, Lane &l, uint8_t *d_out, uint64_t slot_stride) {
    const bool rgb = l.g.planes_per_image == 3;
    if (l.g.depth == FELICS_DEPTH_16) return rgb ? run_wide<int32_t>(ctx, l, d_out, slot_stride) : run_wide<uint16_t>(ctx, l, d_out, slot_stride);
    return rgb ? run_lane<int16_t, uint16_t>(ctx, l, d_out, slot_stride) : run_lane<uint8_t, uint8_t>(ctx, l, d_out, slot_stride);
}

// Queues one sub-batch (cnt frames starting at frame `first` of d_pixels) on a lane: geometry, colour
// transform, and everything run_lane / run_wide enqueue.  Returns without waiting.
int launch_sub_batch(felics_ctx *ctx, Lane &l, size_t first, size_t cnt, const void *d_pixels, uint32_t w, uint32_t h,
                     int color, int depth, uint8_t *lane_out, uint64_t slot, int nslices, bool queued) {
    const Geometry &g = begin_sub_batch(ctx, l, first, cnt, w, h, color, depth, nslices, queued);
    const bool wide = depth == FELICS_DEPTH_16;
    const size_t frame_bytes = (size_t)g.npix * g.planes_per_image * (wide ? 2 : 1);
    int rc;
    const uint8_t *src = (const uint8_t *)d_pixels + first * frame_bytes;
    l.d_planes = src;
    hipStream_t fs = wide || ctx->serial ? l.stream : l.front;  // the stream the sub-batch's first kernel runs on
    if (ctx->wait_before_submit)  // (felics_compress_batch: the frames are still on their way)
        HIP_TRY(ctx, hipStreamWaitEvent(fs, ctx->wait_before_submit, 0));
    if (ctx->profiling) HIP_TRY(ctx, hipEventRecord(l.span_begin, fs));
    if (g.planes_per_image == 3) {
        if ((rc = reserve(ctx, l.planes, (size_t)g.nplanes * g.npix * (wide ? 4 : 2) + STAGE_PAD)) != 0) return rc;
        StageTimer t(ctx, l, ST_PLANES, fs, true);
        if (wide)
            launch_rgb16_to_planes(fs, (const uint16_t *)src, (int32_t *)l.planes.p, g.npix, g.nimages);
        else
            launch_rgb8_to_planes(fs, src, (int16_t *)l.planes.p, g.npix, g.nimages);
        l.d_planes = l.planes.p;
    }
    return run_sub_batch(ctx, l, lane_out, slot);
}

// The device's `error | flags << 32` word of an 8-bit sub-batch (run_lane copies it back behind the sizes).
SlotOutcome decode_status(const felics_ctx *ctx, const Lane &l, uint64_t word) {
    const uint32_t err = (uint32_t)word, flags = (uint32_t)(word >> 32);
    SlotOutcome o;
    o.lookback_failed = (err & 1u) != 0 || (ctx->test_lookback && l.m_fused);
    o.overflow = (err & 2u) != 0;
    o.order_violation = (flags & TL_FLAG_ORDER) != 0;
    o.tile_overflow = (flags & TL_FLAG_OVERFLOW) != 0;
    o.spine_error = (flags & TL_FLAG_SPINE) != 0;
    return o;
}

SlotOutcome read_sizes(felics_ctx *ctx, Lane &l, bool wide, uint64_t slot, uint64_t *offsets, uint64_t *lens) {
    SlotOutcome o;  // (run_wide copies the sizes and nothing else)
    if (!wide) o = decode_status(ctx, l, l.h_sizes[l.g.nimages]);
    for (size_t i = 0; i < l.g.nimages; i++) {
        lens[l.first_image + i] = l.h_sizes[i];
        offsets[l.first_image + i] = (uint64_t)(l.first_image + i) * slot;
        if (slot != 0 && l.h_sizes[i] > slot) o.overflow = true;
    }
    return o;
}

// A tile of the single-pass pack gave up waiting for the tiles before it.  With tiles taken from the workgroup index that can
// be this context's own doing (a predecessor's workgroup not started yet: XCDs dispatch their shares of a grid independently
// and the other lane's kernels share them), so the first remedy is the ticket counter -- same kernel, a tile then only waits
// for workgroups that are running.  If a ticketed pack gives up as well, something else holds the GPU for a second at a time:
// the context packs with the two-pass kernels from then on.
static void note_lookback_failure(felics_ctx *ctx, const Lane &l) {
    ctx->stats.lookback_fallbacks++;
    if (!l.m_tickets) {  // (what the failed sub-batch itself ran with: two queued submissions that fail together both get here)
        if (!ctx->pack_tickets) ctx->stats.ticket_retries++;
        ctx->pack_tickets = true;
        ctx->err = "a tile gave up waiting for its predecessors: this context now hands its pack tiles out by ticket";
    } else {
        ctx->two_pass = true;
        ctx->stats.two_pass = 1;
        ctx->err = "a tile gave up waiting for its predecessors: this context now packs with the two-pass kernels (slower)";
    }
}

// k_front ranks a batch of events with one returning LDS atomic and relies on the lanes that name one address being served in
// lane order -- which this hardware does (profiles/tools/micro/lds_atomic_order.hip) and no document promises; so the kernel
// checks the order of what it wrote, and a context whose check fails once ranks with ballots from then on.
static void note_scatter_order_violation(felics_ctx *ctx) {
    ctx->stats.scatter_fallbacks++;
    ctx->scatter_ballot = true;
    ctx->err = "the front kernel's order check failed: this context now ranks events with ballots";
}

// A tile's events did not fit the slots a tile gets by default: the worst case from now on (more memory, same kernels).
static void note_tile_overflow(felics_ctx *ctx) {
    ctx->stats.tile_overflows++;
    ctx->cap_max = true;
    ctx->test_tile_cap = false;
    ctx->err = "a tile's events outgrew its slots: this context now sizes its tiles for the worst case";
}

static int spine_failure(felics_ctx *ctx) {
    ctx->err = "internal error: the spine's halving search lost its invariant";
    return FELICS_E_HIP;
}

// A sub-batch that is not to be used as it came out (the lane has been waited for): what the context does differently from now
// on, and the counter of the case.  One cause per sub-batch, in this order: the spine's self-check (an error, returned), the front
// kernel's order check, a tile's slots, the look-back, and -- only when nothing else asks for the redo -- a stream's slot.
int apply_remedy(felics_ctx *ctx, const Lane &l, const SlotOutcome &o) {
    if (o.spine_error) return spine_failure(ctx);
    if (o.order_violation)
        note_scatter_order_violation(ctx);
    else if (o.tile_overflow)
        note_tile_overflow(ctx);
    else if (o.lookback_failed)
        note_lookback_failure(ctx, l);
    else if (o.overflow)
        ctx->stats.slot_overflows++;
    return FELICS_OK;
}

// The version-2 restart indexes of a 16-bit pass that has packed and is what the caller gets (felics_compress_batch_device_indexed16;
// launch_index16_scan / _write, felics_kernels.h), from the lane's workspace: the sorted records and chain heads, the tiles' bit offsets,
// the planes.  The size of an index depends on the content, so the host reads the totals between the two steps, places the pass's
// indexes behind the ones before them and has only those written whose end lies inside the caller's buffer.  Queued on the tail
// stream, behind pack_exact where that ran; returns with the tail stream's work queued (the caller's sync_lane waits for it).
static int emit_index16(felics_ctx *ctx, Lane &l, size_t first, Index16Request &rq) {
    const Geometry &g = l.g;
    const Index16Layout L = index16_layout(g.W, g.H, g.color, rq.segment_pixels);
    const size_t cps = (size_t)g.nplanes * L.K;
    const uint32_t wpc = index16_words_per_checkpoint(g.color);
    int rc;
    if ((rc = reserve(ctx, l.i16_bitmap, cps * wpc * 4)) != 0) return rc;
    if ((rc = reserve(ctx, l.i16_prefix, cps * wpc * 4)) != 0) return rc;
    if ((rc = reserve(ctx, l.i16_nrows, cps * 4)) != 0) return rc;
    if ((rc = reserve(ctx, l.i16_rows_off, cps * 8)) != 0) return rc;
    if ((rc = reserve(ctx, l.i16_totals, (size_t)g.nimages * 16)) != 0) return rc;
    if ((rc = reserve(ctx, l.i16_index_off, (size_t)g.nimages * 8)) != 0) return rc;
    hipStream_t s = l.tail;
    if (ctx->poison) {
        DevBuf *bufs[] = {&l.i16_bitmap, &l.i16_prefix, &l.i16_nrows, &l.i16_rows_off, &l.i16_totals, &l.i16_index_off};
        for (DevBuf *b : bufs) HIP_TRY(ctx, hipMemsetAsync(b->p, 0xA5, b->cap, s));
    }
    const Index16Emit e{rq.d_index, (const uint64_t *)l.i16_index_off.p, (uint32_t *)l.i16_bitmap.p, (uint32_t *)l.i16_prefix.p,
                        (uint32_t *)l.i16_nrows.p, (uint64_t *)l.i16_rows_off.p, (uint64_t *)l.i16_totals.p, g.W, g.H, g.npix, g.color,
                        g.planes_per_image, g.nplanes, g.nimages, L.K, rq.segment_pixels, wpc};
    launch_index16_scan(s, (const uint64_t *)l.wrecs[0].p, (const uint32_t *)l.wmeta.p, g, e);
    HIP_TRY(ctx, hipGetLastError());
    std::vector<uint64_t> totals((size_t)g.nimages * 2), where(g.nimages);
    HIP_TRY(ctx, hipMemcpyAsync(totals.data(), l.i16_totals.p, totals.size() * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    uint64_t fit = 0, rows = 0;
    for (size_t i = 0; i < g.nimages; i++) {
        const uint64_t bytes = totals[2 * i];
        rq.idx_offsets[first + i] = rq.total;
        rq.idx_lens[first + i] = bytes;
        const bool fits = bytes <= rq.cap && rq.total <= rq.cap - bytes;
        where[i] = fits ? rq.total : ~0ull;
        if (fits) fit++, rows += totals[2 * i + 1], rq.bytes += bytes;
        else rq.too_small = true;
        rq.total += bytes;  // (rows_base and a row are multiples of 64: so is every offset)
    }
    if (fit == 0) return FELICS_OK;
    HIP_TRY(ctx, hipMemcpyAsync(l.i16_index_off.p, where.data(), where.size() * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));  // (`where` is pageable and leaves scope)
    launch_index16_write(s, l.d_planes, (const uint64_t *)l.wrecs[0].p, (const uint32_t *)l.wmeta.p, (const uint64_t *)l.heads.p,
                         (const uint32_t *)l.scalars.p, (const uint64_t *)l.tile_bitoff.p, l.plane_base, l.plane_base - g.nplanes, g, e);
    HIP_TRY(ctx, hipGetLastError());
    rq.written += fit;
    rq.rows += rows;
    rq.passes++;
    return FELICS_OK;
}

// Encode `n` same-shape frames resident in device memory into d_out (device), on one lane, and wait.
// If d_out is NULL the context's own output buffer is used (and grown).
int encode_device(felics_ctx *ctx, Lane &l, size_t n, const void *d_pixels, uint32_t w, uint32_t h, int color, int depth,
                  uint8_t *d_out, size_t d_out_cap, uint64_t *offsets, uint64_t *lens, uint8_t **used_out, bool start_exact,
                  const IndexRequest *index, Index16Request *index16) {
    const uint32_t planes = color == FELICS_COLOR_RGB ? 3 : 1;
    const uint64_t npix = (uint64_t)w * h;
    const bool wide = depth == FELICS_DEPTH_16;
    if (npix * planes >= 0xE0000000ull) return FELICS_E_UNSUPPORTED;
    if (wide && npix > WIDE_MAX_PLANE_PIXELS) return FELICS_E_UNSUPPORTED;  // an event record keeps the sample index in 29 bits
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const bool own_out = d_out == nullptr;

    if (npix == 0) {
        // (0,_) | (_,0): header + two zero i32 per plane (compression.rs:94-98); nothing to compute
        const size_t sz = 14 + 8 * planes;
        const size_t stride = (sz + 15) & ~(size_t)15;
        const size_t need = stride * n;
        if (own_out) {
            int rc = reserve(ctx, ctx->own, need);
            if (rc) return rc;
            d_out = (uint8_t *)ctx->own.p;
            d_out_cap = ctx->own.cap;
        }
        if (need > d_out_cap) {
            if (n) lens[0] = need;
            return FELICS_E_BUFFER_TOO_SMALL;
        }
        std::vector<uint8_t> tmp(need, 0);
        for (size_t i = 0; i < n; i++) {
            header_bytes(tmp.data() + i * stride, w, h, color, depth);
            offsets[i] = i * stride;
            lens[i] = sz;
        }
        if (need) HIP_TRY(ctx, hipMemcpy(d_out, tmp.data(), need, hipMemcpyHostToDevice));
        if (used_out) *used_out = d_out;
        return FELICS_OK;
    }

    const size_t frame_bytes = (size_t)npix * planes * (wide ? 2 : 1);
    size_t per_pass = max_images_per_pass(npix, planes, depth);
    if (index16) per_pass = std::max<size_t>(1, std::min(per_pass, index16->pass_images));  // (its workspace per checkpoint: the entry point's bound)
    int rc;
    // Placement.  Preferred: every stream gets a fixed slot (stream i at i * slot), so packing needs no
    // size from the host and follows the spine slice by slice.  If a stream outgrows its slot, or the
    // caller's buffer is too small for sensible slots, the streams are placed back to back instead
    // (exact sizes first, then one pack pass).
    uint64_t slot = 0;
    if (own_out) {
        slot = default_slot(frame_bytes);
        if ((rc = reserve(ctx, ctx->own, (size_t)(slot * n))) != 0) return rc;
        d_out = (uint8_t *)ctx->own.p;
        d_out_cap = ctx->own.cap;
    } else {
        slot = (d_out_cap / n) & ~15ull;
        if (slot < 64 || slot < frame_bytes / 4) slot = 0;
    }
    if (start_exact) slot = 0;

    // (at most: ranks from ballots, worst-case tiles, tickets, two-pass, exact placement, and the run that succeeds; a loop that
    // runs out without one is reported, not passed off as a result)
    for (int attempt = 0; attempt < 7; attempt++) {
        size_t done = 0;
        uint64_t out_base = 0;  // exact placement: where the next pass's streams start
        SlotOutcome outcome;
        if (index16) index16->total = index16->written = index16->bytes = index16->rows = index16->passes = 0, index16->too_small = false;
        // passes of up to per_pass frames (one pass unless the batch is huge)
        while (done < n && !outcome.overflow && !outcome.redo()) {
            const size_t cnt = std::min(per_pass, n - done);
            const size_t first = done + cnt;
            if ((rc = launch_sub_batch(ctx, l, done, cnt, d_pixels, w, h, color, depth, d_out + done * slot, slot, ctx->slices_blocking)) != 0) {
                (void)sync_lane(ctx, l);
                return rc;
            }
            if ((rc = wait_event(ctx, l.sized, "stream sizes")) != 0) return rc;
            outcome = read_sizes(ctx, l, wide, slot, offsets, lens);
            if (outcome.spine_error) {
                (void)sync_lane(ctx, l);
                return apply_remedy(ctx, l, outcome);
            }
            if (slot == 0 && !outcome.redo()) {
                // exact placement of this pass: back to back, 16-byte aligned, in image order
                uint64_t need = out_base;
                for (size_t i = done; i < first; i++) {
                    offsets[i] = need;
                    need += (lens[i] + 15) & ~15ull;
                }
                if (own_out) {
                    if (done != 0) return FELICS_E_UNSUPPORTED;  // the host entry points submit one pass at a time
                    if ((rc = reserve(ctx, ctx->own, (size_t)need)) != 0) return rc;  // waits for the device
                    d_out = (uint8_t *)ctx->own.p;
                    d_out_cap = ctx->own.cap;
                }
                if (need > d_out_cap) {
                    (void)sync_lane(ctx, l);
                    lens[0] = need;  // capacity needed so far (a lower bound if more passes would follow)
                    return FELICS_E_BUFFER_TOO_SMALL;
                }
                launch_place_streams(l.tail, (const uint64_t *)l.image_bytes.p, (uint64_t *)l.image_off.p, l.g);
                uint8_t *lane_out = d_out + offsets[l.first_image];
                if (wide)
                    rc = planes == 3 ? pack_exact<int32_t>(ctx, l, lane_out) : pack_exact<uint16_t>(ctx, l, lane_out);
                else
                    rc = planes == 3 ? pack_exact<int16_t>(ctx, l, lane_out) : pack_exact<uint8_t>(ctx, l, lane_out);
                if (rc) {
                    (void)sync_lane(ctx, l);
                    return rc;
                }
                out_base = need;
            }
            if (index && !outcome.redo() && !outcome.overflow) {
                // The pass has packed (in its slots, or exactly just now) and is what the caller gets: its restart indexes, from the
                // run table, the records' states, the tiles' bit offsets and the planes, all still in the lane's workspace.  (A pass
                // that is redone by a remedy comes here again and rewrites them.)
                uint8_t *at = index->d_index + done * index->bytes;
                HIP_TRY(ctx, hipMemsetAsync(at, 0, (size_t)(cnt * index->bytes), l.tail));
                launch_index_emit(l.tail, l.d_planes, (const uint32_t *)l.counts.p, (const uint4 *)l.block_state.p, l.m_cap,
                                  (const uint64_t *)l.tile_bitoff.p, l.plane_base, l.plane_base - l.g.nplanes, l.g, at, index->segment_pixels);
                HIP_TRY(ctx, hipGetLastError());
            }
            if (index16 && !outcome.redo() && !outcome.overflow && (rc = emit_index16(ctx, l, done, *index16)) != 0) {
                (void)sync_lane(ctx, l);
                return rc;
            }
            if ((rc = sync_lane(ctx, l)) != 0) return rc;
            done = first;
        }
        if (!outcome.redo() && !outcome.overflow) {
            collect_timing(ctx, l);
            if (used_out) *used_out = d_out;
            return FELICS_OK;
        }
        if (outcome.redo() && (rc = sync_lane(ctx, l)) != 0) return rc;
        (void)apply_remedy(ctx, l, outcome);  // (a spine error has left above)
        if (!outcome.redo()) slot = 0;  // a stream outgrew its slot: do the batch again with exact placement
    }
    ctx->err = "internal error: the batch was redone with every remedy and still did not complete";
    return FELICS_E_HIP;
}

}  // namespace felics

extern "C" {

int felics_compress_batch_device(felics_ctx *ctx, size_t n, const void *d_pixels, uint32_t w, uint32_t h, int color,
                                 int depth, void *d_out, size_t d_out_cap, uint64_t *offsets, uint64_t *lens) {
    if (!ctx || !offsets || !lens || !d_out || (!d_pixels && n && (uint64_t)w * h)) return FELICS_E_INVALID_ARGUMENT;
    if (ctx->failed) return FELICS_E_HIP;
    int rc = check_args(w, h, color, depth);
    if (rc) return rc;
    if (n == 0) return FELICS_OK;
    if (any_pending(ctx)) return FELICS_E_INVALID_ARGUMENT;  // felics_wait_batch first
    return encode_device(ctx, ctx->lanes[0], n, d_pixels, w, h, color, depth, (uint8_t *)d_out, d_out_cap, offsets, lens,
                         nullptr);
}

int felics_compress_batch_device_indexed(felics_ctx *ctx, size_t n, const void *d_pixels, uint32_t w, uint32_t h, int color, int depth, void *d_out,
                                         size_t d_out_cap, uint32_t segment_pixels, void *d_index, size_t d_index_cap, uint64_t *offsets,
                                         uint64_t *lens) {
    if (!ctx || !offsets || !lens || !d_out || !d_index || (!d_pixels && n && (uint64_t)w * h)) return FELICS_E_INVALID_ARGUMENT;
    if (ctx->failed) return FELICS_E_HIP;
    int rc = check_args(w, h, color, depth);
    if (rc) return rc;
    if (depth != FELICS_DEPTH_8) return FELICS_E_UNSUPPORTED;  // 16-bit streams have no index
    const size_t bytes = felics_index_size(w, h, color, depth, segment_pixels);
    if (bytes == 0 || ((uintptr_t)d_index & 15u)) return FELICS_E_INVALID_ARGUMENT;
    if (n == 0) return FELICS_OK;
    if (any_pending(ctx)) return FELICS_E_INVALID_ARGUMENT;  // felics_wait_batch first
    if (d_index_cap / bytes < n) return FELICS_E_BUFFER_TOO_SMALL;
    const IndexRequest req{(uint8_t *)d_index, bytes, segment_pixels};
    rc = encode_device(ctx, ctx->lanes[0], n, d_pixels, w, h, color, depth, (uint8_t *)d_out, d_out_cap, offsets, lens, nullptr, false, &req);
    if (rc == FELICS_OK && (uint64_t)w * h == 0) {
        // an empty image (K = 0) is encoded on the host and so is its index: the header, every plane its two raw samples long
        uint8_t ih[INDEX_HEADER_BYTES];
        empty_index(ih, w, h, (uint32_t)color, segment_pixels);
        for (size_t i = 0; i < n; i++) HIP_TRY(ctx, hipMemcpy((uint8_t *)d_index + i * bytes, ih, bytes, hipMemcpyHostToDevice));
    }
    return rc;
}

int felics_compress_batch_device_indexed_wide(felics_ctx *ctx, size_t n, const void *d_pixels, uint32_t w, uint32_t h, int color, void *d_out,
                                              size_t d_out_cap, uint32_t segment_pixels, void *d_index, size_t d_index_cap, uint64_t *offsets,
                                              uint64_t *lens, uint64_t *idx_offsets, uint64_t *idx_lens, uint64_t *idx_total) {
    if (!ctx || !d_out || !d_index || (!d_pixels && n && (uint64_t)w * h)) return FELICS_E_INVALID_ARGUMENT;
    if (n && (!offsets || !lens || !idx_offsets || !idx_lens)) return FELICS_E_INVALID_ARGUMENT;
    if (ctx->failed) return FELICS_E_HIP;
    int rc = check_args(w, h, color, FELICS_DEPTH_16);
    if (rc) return rc;
    if (!index_segment_ok(segment_pixels) || ((uintptr_t)d_index & 63u)) return FELICS_E_INVALID_ARGUMENT;
    if (idx_total) *idx_total = 0;
    if (n == 0) return FELICS_OK;
    if (any_pending(ctx)) return FELICS_E_INVALID_ARGUMENT;  // felics_wait_batch first
    const uint32_t planes = color == FELICS_COLOR_RGB ? 3 : 1;
    const uint64_t npix = (uint64_t)w * h;
    Index16Request rq{(uint8_t *)d_index, d_index_cap, segment_pixels, SIZE_MAX, idx_offsets, idx_lens};
    if (npix != 0) {
        // the workspace per checkpoint (bitmap and prefix, a bit and a share of a word per context) bounds the images of a pass, within a
        // quarter of the free device memory -- the 16-bit decoder's rule; an image whose own checkpoints do not fit is refused
        if (npix > 0xFFFFFFFFull) return FELICS_E_UNSUPPORTED;
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        size_t free_b = 0, total_b = 0;
        HIP_TRY(ctx, hipMemGetInfo(&free_b, &total_b));
        const Index16Layout L = index16_layout(w, h, (uint32_t)color, segment_pixels);
        const uint64_t per_image = (uint64_t)planes * L.K * (index16_words_per_checkpoint((uint32_t)color) * 8ull + 12u) + 24u;
        uint64_t budget = free_b / 4;
        for (const Lane &l : ctx->lanes) budget += l.i16_bitmap.cap + l.i16_prefix.cap;  // (what this context holds already is its to use)
        rq.pass_images = (size_t)(budget / per_image);
        if (rq.pass_images == 0) return FELICS_E_UNSUPPORTED;
    }
    rc = encode_device(ctx, ctx->lanes[0], n, d_pixels, w, h, color, FELICS_DEPTH_16, (uint8_t *)d_out, d_out_cap, offsets, lens, nullptr, false,
                       nullptr, &rq);
    if (rc) return rc;
    if (npix == 0) {
        // an empty image (K = 0) is encoded on the host and so is its index: the version-2 header alone, as felics_index16_build writes it
        uint8_t ih[INDEX_HEADER_BYTES];
        empty_index(ih, w, h, (uint32_t)color, segment_pixels);
        ih[IDX_VERSION] = (uint8_t)INDEX16_VERSION;
        ih[IDX_DEPTH] = FELICS_DEPTH_16;
        ih[IDX16_TOTAL] = (uint8_t)INDEX_HEADER_BYTES;
        for (size_t i = 0; i < n; i++) {
            idx_offsets[i] = rq.total;
            idx_lens[i] = INDEX_HEADER_BYTES;
            if (rq.total + INDEX_HEADER_BYTES <= d_index_cap) {
                HIP_TRY(ctx, hipMemcpy((uint8_t *)d_index + rq.total, ih, INDEX_HEADER_BYTES, hipMemcpyHostToDevice));
                rq.written++;
                rq.bytes += INDEX_HEADER_BYTES;
            } else {
                rq.too_small = true;
            }
            rq.total += INDEX_HEADER_BYTES;
        }
    }
    if (idx_total) *idx_total = rq.total;
    felics_index16_emit_stats &st = ctx->i16estats;
    st.streams += n;
    st.rows_written += rq.rows;
    st.index_bytes += rq.bytes;
    st.passes += rq.passes;
    return rq.too_small ? FELICS_E_BUFFER_TOO_SMALL : FELICS_OK;
}

int felics_get_index_wide_emit_stats(const felics_ctx *ctx, felics_index16_emit_stats *out, size_t out_size) {
    return copy_stats(ctx, &felics_ctx::i16estats, out, out_size);
}

int felics_submit_batch_device(felics_ctx *ctx, size_t n, const void *d_pixels, uint32_t w, uint32_t h, int color,
                               int depth, void *d_out, size_t d_out_cap, int *ticket) {
    if (!ctx || !ticket || !d_out || n == 0 || (!d_pixels && (uint64_t)w * h)) return FELICS_E_INVALID_ARGUMENT;
    if (ctx->failed) return FELICS_E_HIP;
    int rc = check_args(w, h, color, depth);
    if (rc) return rc;
    const int L = ctx->next_lane;
    Lane &l = ctx->lanes[L];
    if (l.pending) return FELICS_E_INVALID_ARGUMENT;  // MAX_LANES submissions are in flight: wait for the oldest
    l.p_n = n;
    l.p_pixels = d_pixels;
    l.p_w = w;
    l.p_h = h;
    l.p_color = color;
    l.p_depth = depth;
    l.p_out = (uint8_t *)d_out;
    l.p_cap = d_out_cap;
    l.finished = false;
    l.p_surfaces = false;
    const uint32_t planes = color == FELICS_COLOR_RGB ? 3 : 1;
    const uint64_t npix = (uint64_t)w * h;
    const size_t frame_bytes = (size_t)npix * planes * (depth == FELICS_DEPTH_16 ? 2 : 1);
    uint64_t slot = (d_out_cap / n) & ~15ull;
    if (slot < 64 || slot < frame_bytes / 4) slot = 0;
    if (npix == 0 || npix * planes >= 0xE0000000ull || n > max_images_per_pass(npix, planes, depth) || slot == 0) {
        // not the plain case (fixed slots, one pass): do it now, hand the result over at the wait
        l.r_off.assign(n, 0);
        l.r_len.assign(n, 0);
        l.r_rc = encode_device(ctx, l, n, d_pixels, w, h, color, depth, l.p_out, d_out_cap, l.r_off.data(), l.r_len.data(),
                               nullptr);
        l.finished = true;
    } else {
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        l.p_slot = slot;
        if ((rc = launch_sub_batch(ctx, l, 0, n, d_pixels, w, h, color, depth, l.p_out, slot, ctx->slices_queued, true)) != 0) {
            (void)sync_lane(ctx, l);
            return rc;
        }
    }
    l.pending = true;
    *ticket = L;
    ctx->next_lane = (L + 1) % ctx->nlanes;
    return FELICS_OK;
}

int felics_wait_batch(felics_ctx *ctx, int ticket, uint64_t *offsets, uint64_t *lens) {
    if (!ctx || ticket < 0 || ticket >= ctx->nlanes || !offsets || !lens) return FELICS_E_INVALID_ARGUMENT;
    if (ctx->failed) return FELICS_E_HIP;
    Lane &l = ctx->lanes[ticket];
    if (!l.pending) return FELICS_E_INVALID_ARGUMENT;
    if (!l.finished) {
        // the lane stays marked busy until its kernels are known to have finished: after a timeout nothing may
        // reuse or free its workspace
        const int wrc = wait_event(ctx, l.sized, "stream sizes");
        if (wrc) return wrc;
    }
    l.pending = false;
    if (l.finished) {
        for (size_t i = 0; i < l.p_n; i++) {
            offsets[i] = l.r_off[i];
            lens[i] = l.r_len[i];
        }
        return l.r_rc;
    }
    if (l.p_surfaces) return land_surfaces(ctx, l, offsets, lens);
    int rc;
    const SlotOutcome o = read_sizes(ctx, l, l.p_depth == FELICS_DEPTH_16, l.p_slot, offsets, lens);
    if (!o.redo() && !o.overflow && !o.spine_error) {
        collect_timing(ctx, l);
        return FELICS_OK;
    }
    // the rare cases: pack again on this lane, synchronously (two-pass kernels / exact placement)
    if ((rc = sync_lane(ctx, l)) != 0) return rc;
    if ((rc = apply_remedy(ctx, l, o)) != 0) return rc;
    return encode_device(ctx, l, l.p_n, l.p_pixels, l.p_w, l.p_h, l.p_color, l.p_depth, l.p_out, l.p_cap, offsets, lens,
                         nullptr, o.overflow && !o.redo());
}

// The reference's own call shape: images in host memory in, .felics bytes in host memory out (compression.rs:255-282, :322-371;
// cfelics.rs:24-31).  The batch goes through the submission queue in CHUNKS: the frames of chunk c + 1 are copied to the device
// on a copy stream of its own while chunk c is encoded and the streams of chunk c - 1 are copied back on a third stream, so the
// link is busy in both directions under the kernels (measured, 64 4K gray8 frames from and to page-locked memory: 13.8 ms per
// batch; with the copies on the lanes' own streams 15.6).  (The copies are hipMemcpyAsync from / to the caller's pointers: at the
// link's rate, and asynchronous, if that memory is page-locked -- hipHostMalloc, hipHostRegister, a pinned torch tensor -- and
// through the runtime's staging otherwise.)  A chunk whose streams outgrow their slots and the room the slots leave for exact
// placement is encoded once more, blocking, into a buffer that grows.
int felics_compress_batch(felics_ctx *ctx, size_t n, const void *const *pixels, uint32_t w, uint32_t h, int color,
                          int depth, uint8_t *const *outs, const size_t *caps, size_t *lens) {
    if (!ctx || (n && (!pixels || !outs || !caps || !lens))) return FELICS_E_INVALID_ARGUMENT;
    if (ctx->failed) return FELICS_E_HIP;
    int rc = check_args(w, h, color, depth);
    if (rc) return rc;
    if (n == 0) return FELICS_OK;
    if (any_pending(ctx)) return FELICS_E_INVALID_ARGUMENT;  // felics_wait_batch first
    const uint32_t planes = color == FELICS_COLOR_RGB ? 3 : 1;
    const size_t frame_bytes = (size_t)w * h * planes * (depth == FELICS_DEPTH_16 ? 2 : 1);
    for (size_t i = 0; i < n && frame_bytes; i++)
        if (!pixels[i]) return FELICS_E_INVALID_ARGUMENT;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (!ctx->copy_in) {
        HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->copy_in, hipStreamNonBlocking));
        HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->copy_out, hipStreamNonBlocking));
    }
    const size_t per_pass = max_images_per_pass((uint64_t)w * h, planes, depth);
    // chunks: eight per batch (the first chunk's way in and the last one's way out are what the kernels cannot cover), none larger
    // than a pass; a stream's slot as encode_device sizes it
    const size_t chunk = std::max<size_t>(1, std::min(per_pass, (n + 7) / 8));
    const uint64_t slot = default_slot(frame_bytes);
    if ((rc = reserve(ctx, ctx->in, frame_bytes * n + 64)) != 0) return rc;
    if ((rc = reserve(ctx, ctx->out, (size_t)(slot * n) + 64)) != 0) return rc;
    struct Flying {
        int ticket;
        size_t first, cnt;
    };
    std::vector<Flying> flying;
    std::vector<uint64_t> offs(chunk), sizes(chunk);
    int result = FELICS_OK;
    auto land = [&](const Flying &f) -> int {  // wait for a chunk and start its streams on their way to the caller
        int r = felics_wait_batch(ctx, f.ticket, offs.data(), sizes.data());
        const uint8_t *from = (const uint8_t *)ctx->out.p + f.first * slot;
        hipStream_t cs = ctx->copy_out;
        if (r == FELICS_E_BUFFER_TOO_SMALL) {
            // The chunk's streams outgrew their slots AND the room the slots leave for exact placement (16-bit noise: a code can be
            // 2^17 bits): once more, blocking, into a buffer of the library's own that grows to what the streams need.
            Lane &l = ctx->lanes[f.ticket];
            uint8_t *d_own = nullptr;
            r = encode_device(ctx, l, f.cnt, (const uint8_t *)ctx->in.p + f.first * frame_bytes, w, h, color, depth, nullptr, 0, offs.data(),
                              sizes.data(), &d_own);
            from = d_own;
            cs = l.stream;  // (copied out before anything else may touch ctx->own: synchronised below)
        }
        if (r) return r;
        for (size_t i = 0; i < f.cnt; i++) {
            lens[f.first + i] = (size_t)sizes[i];
            if (sizes[i] > caps[f.first + i] || !outs[f.first + i]) {
                result = FELICS_E_BUFFER_TOO_SMALL;  // lens[] still reports every size needed
                continue;
            }
            HIP_TRY(ctx, hipMemcpyAsync(outs[f.first + i], from + offs[i], (size_t)sizes[i], hipMemcpyDeviceToHost, cs));
        }
        if (from != (const uint8_t *)ctx->out.p + f.first * slot) HIP_TRY(ctx, hipStreamSynchronize(cs));
        return FELICS_OK;
    };
    auto drain = [&](int r) {  // an error: nothing of this context may be left in flight behind the caller's back
        for (const Flying &f : flying) (void)felics_wait_batch(ctx, f.ticket, offs.data(), sizes.data());
        (void)hipStreamSynchronize(ctx->copy_in);
        (void)hipStreamSynchronize(ctx->copy_out);
        return r;
    };
    // All frames are put on their way at once, chunk by chunk with an event behind each chunk: the copy stream then runs back to
    // back at the link's rate whatever the host is waiting for (with a chunk's copies queued only when its turn came, the stream
    // stood idle while the host waited for an older chunk's kernels: 35 GB/s instead of the link's ~50).
    // (Eight chunks of a 64-frame batch: a chunk's kernels take ~2 ms whatever its size -- the chain of a single frame -- so with two
    // chunks in flight sixteen chunks are 16 ms of kernels, four leave the first and the last chunk's 2.5 ms of copying uncovered;
    // a short last chunk changed nothing: profiles/r05/experiments.txt.)
    std::vector<size_t> starts;
    for (size_t first = 0; first < n; first += chunk) starts.push_back(first);
    const size_t nchunks = starts.size();
    starts.push_back(n);
    while (ctx->h2d_done.size() < nchunks) {
        hipEvent_t ev = nullptr;
        HIP_TRY(ctx, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        ctx->h2d_done.push_back(ev);
    }
    for (size_t c = 0; c < nchunks; c++) {
        const size_t first = starts[c], cnt = starts[c + 1] - first;
        for (size_t i = 0; i < cnt && frame_bytes; i++) {
            const hipError_t e = hipMemcpyAsync((uint8_t *)ctx->in.p + (first + i) * frame_bytes, pixels[first + i], frame_bytes,
                                                hipMemcpyHostToDevice, ctx->copy_in);
            if (e != hipSuccess) return drain(hip_fail(ctx, e, "copying frames to the device"));
        }
        if (hipEventRecord(ctx->h2d_done[c], ctx->copy_in) != hipSuccess) return drain(hip_fail(ctx, hipGetLastError(), "hipEventRecord"));
    }
    for (size_t c = 0; c < nchunks; c++) {
        const size_t first = starts[c], cnt = starts[c + 1] - first;
        if ((int)flying.size() == ctx->nlanes) {  // every lane is busy: the oldest chunk first (its lane is the next to be used)
            rc = land(flying.front());
            flying.erase(flying.begin());
            if (rc) return drain(rc);
        }
        ctx->wait_before_submit = ctx->h2d_done[c];  // the chunk's first kernel waits for its frames (launch_sub_batch)
        int ticket = -1;
        rc = felics_submit_batch_device(ctx, cnt, (const uint8_t *)ctx->in.p + first * frame_bytes, w, h, color, depth,
                                        (uint8_t *)ctx->out.p + first * slot, (size_t)(slot * cnt), &ticket);
        ctx->wait_before_submit = nullptr;
        if (rc) return drain(rc);
        flying.push_back(Flying{ticket, first, cnt});
    }
    while (!flying.empty()) {
        rc = land(flying.front());
        flying.erase(flying.begin());
        if (rc) return drain(rc);
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->copy_out));  // the streams have landed
    return result;
}

int felics_compress(felics_ctx *ctx, const void *pixels, uint32_t w, uint32_t h, int color, int depth, uint8_t *out,
                    size_t cap, size_t *out_len) {
    if (!out_len) return FELICS_E_INVALID_ARGUMENT;
    const void *px[1] = {pixels};
    uint8_t *outs[1] = {out};
    size_t caps[1] = {cap};
    size_t lens[1] = {0};
    if (!pixels && (uint64_t)w * h != 0) return FELICS_E_INVALID_ARGUMENT;
    static const uint8_t dummy = 0;
    if (!pixels) px[0] = &dummy;
    int rc = felics_compress_batch(ctx, 1, px, w, h, color, depth, outs, caps, lens);
    *out_len = lens[0];
    return rc;
}

}  // extern "C"
