// lanewalk_check.cpp -- host check of felics_lanewalk.h, the per-lane code of k_decode8_lanes, k_decode8_seg_lanes and k_decode16_lanes:
// the very functions the kernels compile decode one stream per call, with what a kernel does around them (reader and estimator set-up,
// the status) written out here.  Every buffer a walk may touch is allocated at exactly that size -- the stream to the aligned dwords
// that hold it, a plane to its last sample, a pitched view to the last row's W-th sample, a table to its rows, the estimator's "LDS
// column" from a lane's first dword to its last -- so that under AddressSanitizer (make asan) any access beyond them
// is a report; there the samples inside a buffer that are not the walk's (a view's gaps, a plane outside the segment) are poisoned
// while it runs, as far as the sanitizer's eight-byte granules allow, so that a LOAD of them is a report too.  Streams come from the
// oracle's encoder on images made here.  tests/test_lanewalk.py runs both builds; exit status 0 and a last line "all checks held" =
// every check held, otherwise the first failure is named.
#include <sanitizer/asan_interface.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <type_traits>
#include <vector>

static unsigned long note_cold, note_long_code;  // pixels whose context row came from the table; pixels whose Rice code took the long path
#define FELICS_LANEWALK_NOTE(what) ((void)++note_##what)

#include "../../oracle/felics_oracle.h"
#include "felics_index.h"
#include "felics_lanewalk.h"

using namespace felics;

#define FAIL(...)                 \
    do {                          \
        printf("FAILED: ");       \
        printf(__VA_ARGS__);      \
        printf("\n");             \
        exit(1);                  \
    } while (0)

static uint32_t lcg_state = 12345;
static uint32_t lcg() {
    lcg_state = lcg_state * 1664525u + 1013904223u;
    return lcg_state >> 8;
}

enum Kind { NOISE, FLAT, CHECKER, RAMP, SPIKES, KINDS };
static const char *const KIND_NAME[KINDS] = {"noise", "flat", "checker", "ramp", "spikes"};
// w x h x ch samples of 0 .. maxv.  noise: half the samples anywhere in the range, half within 0 .. 3 -- quiet stretches teach the small
// contexts k = 0, so a loud sample behind one is a long code, and loud neighbours are contexts far beyond the hot ones
static std::vector<uint16_t> image(Kind kind, uint32_t w, uint32_t h, uint32_t ch, uint32_t maxv) {
    std::vector<uint16_t> px((size_t)w * h * ch);
    for (uint32_t y = 0; y < h; y++)
        for (uint32_t x = 0; x < w; x++)
            for (uint32_t c = 0; c < ch; c++) {
                uint32_t v = 0;
                switch (kind) {
                    case NOISE: v = (lcg() & 1) ? lcg() % (maxv + 1) : lcg() & 3; break;
                    case FLAT: v = maxv / 3 + c; break;
                    case CHECKER: v = ((x + y + c) & 1) ? maxv : 0; break;
                    case RAMP: v = (x * 3 + y * 5 + c * 7 + (lcg() & 1)) % (maxv + 1); break;
                    default: v = lcg() % 23 == 0 ? maxv - (lcg() & 7) : 40 + (lcg() & 1); break;
                }
                px[((size_t)y * w + x) * ch + c] = (uint16_t)v;
            }
    return px;
}

// the stream of an image (the oracle's encoder); depth 0: the samples as bytes
static std::vector<uint8_t> compress(const std::vector<uint16_t> &px, uint32_t w, uint32_t h, int color, int depth) {
    std::vector<uint8_t> bytes(px.begin(), px.end());
    std::vector<uint8_t> out(fo_max_compressed_size(w, h, color, depth));
    size_t len = 0;
    const int rc = fo_compress(depth ? (const void *)px.data() : (const void *)bytes.data(), w, h, color, depth, out.data(), out.size(), &len);
    if (rc != FO_OK) FAIL("fo_compress %u x %u: %d", w, h, rc);
    out.resize(len);
    return out;
}
// plane c of an image as the decoders' planes hold it: gray as it is, RGB as Y / Co / Cg
static std::vector<int32_t> plane_of(const std::vector<uint16_t> &px, size_t npix, int color, uint32_t c) {
    std::vector<int32_t> p(npix);
    for (size_t i = 0; i < npix; i++) {
        if (!color) {
            p[i] = px[i];
        } else {
            int32_t ycc[3];
            fo_rgb_to_ycocg(px[3 * i], px[3 * i + 1], px[3 * i + 2], &ycc[0], &ycc[1], &ycc[2]);
            p[i] = ycc[c];
        }
    }
    return p;
}

// A stream as a lane may read it: the aligned dwords that hold its bytes and nothing else.  The first byte's alignment goes round.
struct StreamCopy {
    std::unique_ptr<uint32_t[]> dw;
    const uint8_t *s;
    StreamCopy(const uint8_t *bytes, size_t len) {
        static uint32_t turn;
        const uint32_t skew = turn++ & 3u;
        dw.reset(new uint32_t[(skew + len + 3) / 4]());
        memcpy(reinterpret_cast<uint8_t *>(dw.get()) + skew, bytes, len);
        s = reinterpret_cast<const uint8_t *>(dw.get()) + skew;
    }
};
// the estimator column of one lane in a wave's LDS block, from the lane's first dword to its last: dword i at myhot[i * 64]
struct HotColumn {
    std::unique_ptr<uint32_t[]> block{new uint32_t[(DEC8L_HOT * 3 - 1) * 64 + 1]()};
    uint32_t *myhot = block.get();
};

// ---- what k_decode8_lanes / k_decode16_lanes do with one stream whose header matched: the planes one after the other off one reader.
// plane(c): where plane c goes.  Returns the lane's status.
template <bool RGB, bool PITCHED, typename ST, typename PlaneAt>
static int walk8(const uint8_t *bytes, size_t len, uint32_t W, uint32_t H, int64_t pitch, PlaneAt plane) {
    const StreamCopy sc(bytes, len);
    int rc = FELICS_OK;
    LaneReader br;
    br.init(sc.s + FELICS_HEADER_BYTES, len - FELICS_HEADER_BYTES);
    HotColumn hot;
    Lane8Step<RGB> step{{hot.myhot, nullptr}, 0};
    for (uint32_t c = 0; c < (RGB ? 3u : 1u); c++) {
        for (uint32_t i = 0; i < DEC8L_HOT * 3; i++) step.est.myhot[i * 64] = 0;
        const int32_t p0 = (int32_t)br.get(32), p1 = (int32_t)br.get(32);
        if (br.failed() && rc == FELICS_OK) rc = FELICS_E_IO;
        const std::unique_ptr<uint32_t[]> tab(new uint32_t[RGB ? DEC8L_TABLE_DW_RGB : DEC8L_TABLE_DW]());
        step.est.tab = tab.get();
        lane_walk_plane<ST, PITCHED>(br, step, plane(c), pitch, W, H, p0, p1, rc);
    }
    if (br.failed() && rc == FELICS_OK) rc = FELICS_E_IO;
    return rc;
}
// (kept: a table that outlives the call, as a slot's rows of dec_lane16_table outlive a launch, and the first of the call's epochs --
// otherwise every plane gets zeroed rows of its own)
template <bool RGB, bool PITCHED, typename ST, typename PlaneAt>
static int walk16(const uint8_t *bytes, size_t len, uint32_t W, uint32_t H, int64_t pitch, PlaneAt plane, LaneQuad *kept = nullptr, uint32_t epoch0 = 7) {
    const StreamCopy sc(bytes, len);
    int rc = FELICS_OK;
    LaneReader br;
    br.init(sc.s + FELICS_HEADER_BYTES, len - FELICS_HEADER_BYTES);
    const uint32_t rows = dec16l_rows((uint64_t)W * H, RGB ? 3u : 1u);
    for (uint32_t c = 0; c < (RGB ? 3u : 1u); c++) {
        const int32_t p0 = (int32_t)br.get(32), p1 = (int32_t)br.get(32);
        if (br.failed() && rc == FELICS_OK) rc = FELICS_E_IO;
        const std::unique_ptr<LaneQuad[]> tab(new LaneQuad[kept ? 0 : (size_t)rows * 4]());
        Lane16Step step{kept ? kept + (size_t)c * rows * 4 : tab.get(), rows, epoch0 + c, (RGB && c > 0) ? -65535 : 0, 65535, 0};
        lane_walk_plane<ST, PITCHED>(br, step, plane(c), pitch, W, H, p0, p1, rc);
    }
    if (br.failed() && rc == FELICS_OK) rc = FELICS_E_IO;
    return rc;
}
// a dense stream into exact planes; -> status, the planes in `got`
template <typename ST>
static int walk_dense(const std::vector<uint8_t> &st, uint32_t W, uint32_t H, int color, int depth, std::vector<std::vector<int32_t>> &got) {
    const size_t npix = (size_t)W * H;
    const uint32_t np = color ? 3u : 1u;
    std::vector<std::unique_ptr<ST[]>> planes;
    for (uint32_t c = 0; c < np; c++) planes.emplace_back(new ST[npix]());
    const auto at = [&](uint32_t c) { return planes[c].get(); };
    int rc;
    if constexpr (sizeof(ST) == 1) rc = walk8<false, false, ST>(st.data(), st.size(), W, H, 0, at);
    else if constexpr (std::is_same<ST, int16_t>::value) rc = walk8<true, false, ST>(st.data(), st.size(), W, H, 0, at);
    else if constexpr (std::is_same<ST, uint16_t>::value) rc = walk16<false, false, ST>(st.data(), st.size(), W, H, 0, at);
    else rc = walk16<true, false, ST>(st.data(), st.size(), W, H, 0, at);
    (void)depth;
    got.assign(np, std::vector<int32_t>(npix));
    for (uint32_t c = 0; c < np; c++)
        for (size_t i = 0; i < npix; i++) got[c][i] = (int32_t)planes[c][i];
    return rc;
}
static int walk_any(const std::vector<uint8_t> &st, uint32_t W, uint32_t H, int color, int depth, std::vector<std::vector<int32_t>> &got) {
    if (!depth) return color ? walk_dense<int16_t>(st, W, H, color, depth, got) : walk_dense<uint8_t>(st, W, H, color, depth, got);
    return color ? walk_dense<int32_t>(st, W, H, color, depth, got) : walk_dense<uint16_t>(st, W, H, color, depth, got);
}

static const uint32_t WIDTHS[] = {8, 9, 10, 11, 12, 13, 16, 67}, HEIGHTS[] = {1, 2, 3, 6};

static void whole_planes() {
    unsigned long streams = 0, cold[KINDS] = {0}, longc[KINDS][2] = {{0}};  // long codes by depth: each step has its own limit
    for (int kind = 0; kind < KINDS; kind++)
        for (uint32_t W : WIDTHS)
            for (uint32_t H : HEIGHTS)
                for (int depth = 0; depth < 2; depth++)
                    for (int color = 0; color < 2; color++) {
                        const std::vector<uint16_t> px = image((Kind)kind, W, H, color ? 3 : 1, depth ? 65535 : 255);
                        const std::vector<uint8_t> st = compress(px, W, H, color, depth);
                        note_cold = note_long_code = 0;
                        std::vector<std::vector<int32_t>> got;
                        const int rc = walk_any(st, W, H, color, depth, got);
                        if (rc != FELICS_OK) FAIL("whole planes: %s %u x %u colour %d depth %d: status %d", KIND_NAME[kind], W, H, color, depth, rc);
                        for (uint32_t c = 0; c < got.size(); c++)
                            if (got[c] != plane_of(px, (size_t)W * H, color, c))
                                FAIL("whole planes: %s %u x %u colour %d depth %d: plane %u differs", KIND_NAME[kind], W, H, color, depth, c);
                        streams++;
                        cold[kind] += note_cold;
                        longc[kind][depth] += note_long_code;
                    }
    for (int kind = 0; kind < KINDS; kind++)
        printf("whole planes: %s cold-context pixels %lu long-code pixels 8-bit %lu 16-bit %lu\n", KIND_NAME[kind], cold[kind], longc[kind][0], longc[kind][1]);
    if (!cold[NOISE] || !longc[NOISE][0] || !longc[NOISE][1])
        FAIL("whole planes: the noise images did not reach the cold contexts or, in the 8-bit and in the 16-bit step, the long codes");
    printf("whole planes: %lu streams decoded to their originals\n", streams);
}

// gray into a view of `pitch` samples a row that ends with the last row's W-th sample; the gaps keep their pattern
template <typename ST>
static void pitched_one(Kind kind, uint32_t W, uint32_t H, uint32_t extra) {
    const int depth = sizeof(ST) == 2;
    const std::vector<uint16_t> px = image(kind, W, H, 1, depth ? 65535 : 255);
    const std::vector<uint8_t> st = compress(px, W, H, 0, depth);
    const int64_t pitch = W + extra;
    const size_t n = (size_t)(H - 1) * pitch + W;
    const ST pattern = (ST)0xA5A5;
    const std::unique_ptr<ST[]> view(new ST[n]);
    for (size_t i = 0; i < n; i++) view[i] = pattern;
    for (uint32_t y = 0; y + 1 < H; y++) ASAN_POISON_MEMORY_REGION(&view[y * pitch + W], extra * sizeof(ST));
    const auto at = [&](uint32_t) { return view.get(); };
    const int rc = depth ? walk16<false, true, ST>(st.data(), st.size(), W, H, pitch, at) : walk8<false, true, ST>(st.data(), st.size(), W, H, pitch, at);
    ASAN_UNPOISON_MEMORY_REGION(view.get(), n * sizeof(ST));
    if (rc != FELICS_OK) FAIL("pitched: %s %u x %u pitch %ld depth %d: status %d", KIND_NAME[kind], W, H, (long)pitch, depth, rc);
    for (size_t i = 0; i < n; i++) {
        const size_t x = i % pitch, y = i / pitch;
        if (x < W ? view[i] != (ST)px[y * W + x] : view[i] != pattern)
            FAIL("pitched: %s %u x %u pitch %ld depth %d: %s at row %zu sample %zu", KIND_NAME[kind], W, H, (long)pitch, depth,
                 x < W ? "wrong sample" : "gap written", y, x);
    }
}
static void pitched() {
    unsigned long views = 0;
    for (Kind kind : {NOISE, RAMP, SPIKES})
        for (uint32_t W : WIDTHS)
            for (uint32_t H : HEIGHTS)
                for (uint32_t extra : {1u, 7u}) {
                    pitched_one<uint8_t>(kind, W, H, extra);
                    pitched_one<uint16_t>(kind, W, H, extra);
                    views += 2;
                }
    printf("pitched: %lu views decoded, their gaps untouched\n", views);
}

// ---- what a lane of k_decode8_seg_lanes does with segment (c, j) of a stream whose checks passed: into a plane that holds a pattern
// outside the segment.  Returns the status word.
template <bool RGB>
static int walk_segment(const uint8_t *bytes, size_t len, const uint8_t *index_bytes, size_t index_len, uint32_t W, uint32_t H, uint32_t seg,
                        uint32_t c, uint32_t j, const std::vector<int32_t> &want, const char *what) {
    using ST = typename std::conditional<RGB, int16_t, uint8_t>::type;
    constexpr uint32_t TABLE_DW = RGB ? DEC8L_TABLE_DW_RGB : DEC8L_TABLE_DW;
    const StreamCopy sc(bytes, len);
    const std::unique_ptr<uint64_t[]> index(new uint64_t[index_len / 8]);  // (a multiple of 16 bytes)
    memcpy(index.get(), index_bytes, index_len);
    const uint8_t *idx = reinterpret_cast<const uint8_t *>(index.get());
    IndexLayout L;
    uint64_t start = 0, end = 0;
    if (index_header_check(idx, RGB, W, H, len, L) != FELICS_OK || L.total != index_len || index_segment_bounds(idx, L, c, j, len, start, end) != FELICS_OK)
        FAIL("%s: the index's own checks failed", what);
    const uint64_t npix = (uint64_t)W * H, p0 = (uint64_t)j * seg, pend = lane_min<uint64_t>(npix, p0 + seg);
    const uint8_t *cp = idx + INDEX_HEADER_BYTES + ((uint64_t)c * L.K + j) * L.cp_bytes;
    const ST *win = reinterpret_cast<const ST *>(cp + L.win_off);
    // the estimator LOADED: the state's hot rows into the column, its rows into the table
    HotColumn hot;
    const std::unique_ptr<uint32_t[]> tab(new uint32_t[TABLE_DW]);
    memcpy(tab.get(), cp + CP_STATE_OFF, TABLE_DW * 4);
    for (uint32_t i = 0; i < DEC8L_HOT * 3; i++) hot.myhot[i * 64] = tab[i];
    const Lane8Estimator est{hot.myhot, tab.get()};
    const ST pattern = (ST)0x5A5A;
    const std::unique_ptr<ST[]> out(new ST[npix]);
    for (uint64_t i = 0; i < npix; i++) out[i] = pattern;
    int rc = FELICS_OK;
    LaneReader br;
    br.init_at(sc.s, len, start);
    int32_t raw0 = 0, raw1 = 0;
    if (j == 0) {
        raw0 = (int32_t)br.get(32);
        raw1 = (int32_t)br.get(32);
        if (br.failed()) rc = FELICS_E_IO;
    }
    ASAN_POISON_MEMORY_REGION(out.get(), p0 * sizeof(ST));
    ASAN_POISON_MEMORY_REGION(out.get() + pend, (npix - pend) * sizeof(ST));
    const uint32_t out_of_range = lane8_walk_segment<RGB>(br, est, out.get(), win, W, p0, pend, raw0, raw1, rc);
    ASAN_UNPOISON_MEMORY_REGION(out.get(), npix * sizeof(ST));
    if (br.failed()) rc = FELICS_E_IO;
    else if (rc == FELICS_OK && lane8_bad<RGB>(out_of_range)) rc = FELICS_E_INVALID_VALUE;
    else if (rc == FELICS_OK && br.bit_pos(sc.s) != end) rc = FELICS_E_INVALID_INDEX;
    for (uint64_t i = 0; i < npix; i++)
        if (i >= p0 && i < pend ? (int32_t)out[i] != want[i] : out[i] != pattern)
            FAIL("%s plane %u segment %u: %s at pixel %llu", what, c, j, i >= p0 && i < pend ? "wrong sample" : "written outside the segment",
                 (unsigned long long)i);
    return rc;
}

static void from_checkpoints() {
    // tests/test_index_lanes_gpu.py's SHAPES, and odd widths whose segments of 4096 start mid-row at x & 3 = 0, 1, 2 and 3
    static const uint32_t SHAPES[][2] = {{64, 65}, {99, 130}, {9, 1000}, {8, 600}, {4097, 1}, {5000, 3}, {8200, 2}, {4096, 3}, {512, 256},
                                         {9, 2000}, {11, 3400}, {13, 1300}};
    unsigned long segments = 0;
    uint32_t starts[4] = {0, 0, 0, 0};
    for (const auto &shape : SHAPES)
        for (int color = 0; color < 2; color++) {
            const uint32_t W = shape[0], H = shape[1];
            // quiet rows first (halvings before the later checkpoints), then noise
            std::vector<uint16_t> px = image(RAMP, W, H, color ? 3 : 1, 255);
            const std::vector<uint16_t> loud = image(NOISE, W, H, color ? 3 : 1, 255);
            std::copy(loud.begin() + loud.size() / 2, loud.end(), px.begin() + px.size() / 2);
            const std::vector<uint8_t> st = compress(px, W, H, color, 0);
            for (uint32_t seg : {4096u, 12288u}) {
                std::vector<uint8_t> index(felics_index_size(W, H, color, 0, seg));
                size_t ilen = 0;
                if (felics_index_build(st.data(), st.size(), seg, index.data(), index.size(), &ilen) != FELICS_OK || ilen != index.size())
                    FAIL("from a checkpoint: felics_index_build %u x %u", W, H);
                const uint32_t K = (uint32_t)(((uint64_t)W * H + seg - 1) / seg);
                char what[96];
                snprintf(what, sizeof what, "from a checkpoint: %u x %u colour %d segment %u", W, H, color, seg);
                for (uint32_t c = 0; c < (color ? 3u : 1u); c++) {
                    const std::vector<int32_t> want = plane_of(px, (size_t)W * H, color, c);
                    for (uint32_t j = 0; j < K; j++) {
                        const int rc = color ? walk_segment<true>(st.data(), st.size(), index.data(), ilen, W, H, seg, c, j, want, what)
                                             : walk_segment<false>(st.data(), st.size(), index.data(), ilen, W, H, seg, c, j, want, what);
                        if (rc != FELICS_OK) FAIL("%s plane %u segment %u: status %d", what, c, j, rc);
                        segments++;
                        const uint32_t x0 = (uint32_t)(((uint64_t)j * seg) % W);
                        if ((W & 1) && x0) starts[x0 & 3]++;
                    }
                }
            }
        }
    if (!starts[0] || !starts[1] || !starts[2] || !starts[3]) FAIL("from a checkpoint: no odd-width segment starts mid-row at every x & 3");
    printf("from a checkpoint: %lu segments decoded inside their pixels, end checks held (odd widths, mid-row starts at x & 3 = 0..3: %u %u %u %u)\n",
           segments, starts[0], starts[1], starts[2], starts[3]);
}

// cut and flipped gray streams: where the host decoder fails the walk's status is nonzero; where the walk reports OK the pixels are
// the host decoder's
static void damage() {
    unsigned long flips = 0, host_ok_flips = 0, cuts = 0;
    const struct {
        Kind kind;
        uint32_t W, H;
        int depth;
    } sets[] = {{NOISE, 67, 6, 0}, {RAMP, 16, 6, 0}, {SPIKES, 13, 3, 0}, {NOISE, 67, 6, 1}, {RAMP, 11, 3, 1}};
    for (const auto &t : sets) {
        const std::vector<uint16_t> px = image(t.kind, t.W, t.H, 1, t.depth ? 65535 : 255);
        const std::vector<uint8_t> good = compress(px, t.W, t.H, 0, t.depth);
        const size_t npix = (size_t)t.W * t.H;
        std::vector<std::vector<uint8_t>> bad;
        for (size_t cut : {(size_t)FELICS_HEADER_BYTES, good.size() / 2, good.size() - 1}) bad.emplace_back(good.begin(), good.begin() + cut);
        cuts += bad.size();
        for (int f = 0; f < 40; f++) {
            bad.push_back(good);
            bad.back()[FELICS_HEADER_BYTES + lcg() % (good.size() - FELICS_HEADER_BYTES)] ^= (uint8_t)(1u << (lcg() & 7));
        }
        for (size_t b = 0; b < bad.size(); b++) {
            std::vector<uint16_t> host(npix);
            felics_header hdr;
            const bool host_ok = felics_decompress(bad[b].data(), bad[b].size(), host.data(), npix * (t.depth ? 2 : 1), &hdr) == FELICS_OK;
            std::vector<std::vector<int32_t>> got;
            const int rc = walk_any(bad[b], t.W, t.H, 0, t.depth, got);
            if (b >= 3) {
                flips++;
                host_ok_flips += host_ok;
            }
            if (!host_ok && rc == FELICS_OK) FAIL("damage: %s depth %d stream %zu: the host decoder fails, the walk reports OK", KIND_NAME[t.kind], t.depth, b);
            if (rc == FELICS_OK)
                for (size_t i = 0; i < npix; i++) {
                    const int32_t want = t.depth ? (int32_t)host[i] : (int32_t)reinterpret_cast<const uint8_t *>(host.data())[i];
                    if (got[0][i] != want) FAIL("damage: %s depth %d stream %zu: OK with other pixels than the host decoder's", KIND_NAME[t.kind], t.depth, b);
                }
        }
    }
    printf("damage: %lu cut streams, %lu bit flips of which the host decoder still decodes %lu (%.0f %%)\n", cuts, flips, host_ok_flips,
           100.0 * host_ok_flips / flips);
    if (host_ok_flips == flips) FAIL("damage: no flip fails on the host: another seed is needed");
}

// The rows a launch leaves are another launch's only while the epochs differ or a clear lies between (felics_epochs.h): 8 x 8 gray16
// frames whose samples are a few widely spaced values -- every pixel out of range, the same few contexts again and again, large
// errors -- decoded into the rows ANOTHER such frame left in the SAME epoch, nothing between, come out wrong; in another epoch, or
// behind a clear, they come out right.  (Whether such rows are still there after a whole period of epochs is whole_cycle's question.)
static void stale_table() {
    constexpr uint32_t W = 8, H = 8, FRAMES = 300, APART = 8;
    const uint32_t rows = dec16l_rows((uint64_t)W * H, 1);
    std::vector<std::vector<uint16_t>> px(FRAMES);
    std::vector<std::vector<uint8_t>> st(FRAMES);
    for (uint32_t i = 0; i < FRAMES; i++) {
        px[i].resize(W * H);
        for (uint16_t &v : px[i]) v = (uint16_t)((lcg() & 15u) * 4096u);
        st[i] = compress(px[i], W, H, 0, 1);
    }
    const std::unique_ptr<LaneQuad[]> tab(new LaneQuad[(size_t)rows * 4]);
    const std::unique_ptr<uint16_t[]> out(new uint16_t[W * H]);
    const auto at = [&](uint32_t) { return out.get(); };
    const auto decodes = [&](uint32_t i, uint32_t epoch) {
        const int rc = walk16<false, false, uint16_t>(st[i].data(), st[i].size(), W, H, 0, at, tab.get(), epoch);
        return rc == FELICS_OK && std::equal(px[i].begin(), px[i].end(), out.get());
    };
    unsigned long wrong = 0;
    for (uint32_t i = 0; i < FRAMES; i++) {
        const uint32_t later = (i + APART) % FRAMES;
        memset(tab.get(), 0, (size_t)rows * 4 * sizeof(LaneQuad));
        if (!decodes(i, 1)) FAIL("stale table: frame %u on zeroed rows", i);
        wrong += !decodes(later, 1);  // the same epoch, no clear: frame i's counters pass for this frame's
        memset(tab.get(), 0, (size_t)rows * 4 * sizeof(LaneQuad));
        if (!decodes(i, 1) || !decodes(later, 2)) FAIL("stale table: frame %u behind frame %u in another epoch", later, i);
        memset(tab.get(), 0, (size_t)rows * 4 * sizeof(LaneQuad));
        if (!decodes(later, 1)) FAIL("stale table: frame %u behind a clear", later);
    }
    printf("stale table: %lu of %u frames decode wrongly on the rows another frame left in the same epoch; none in another epoch or behind a clear\n", wrong,
           FRAMES);
    if (wrong * 10 < FRAMES * 9) FAIL("stale table: fewer than nine in ten of these frames notice stale rows");
}

// ---- the whole cycle of the lane form's epochs in one slot, as tests/test_gpu_epochs.py runs it on the GPU, on a table that is NEVER
// cleared: launches 1 .. 10 922 in epochs 1, 4, 7, ..., launch 10 923 in epoch 1 again.  A row of another epoch is an empty row and is
// reclaimed by whoever probes it, so launch 1's rows survive 10 921 launches only where those never probe: launches 1 and 10 923
// decode "edge" frames (samples k * CYCLE_EDGE_STEP: contexts of their own), the launches between them "middle" frames (k * 4096),
// whose sixteen contexts and probe rows leave most of the edge contexts' rows alone.  The simulation must find launch 10 923 decoding
// wrongly in at least half the slots (one is enough for the GPU test to fail; measured: all 64, nine or ten rows of launch 1 left in
// each) -- and rightly once the table is cleared in front of it; it also counts what a schedule of middle frames alone
// would leave (nothing: every row reclaimed).  The frames come from cycle_frame, which the GPU test writes out again in Python.
constexpr uint32_t CYCLE_EDGE_STEP = 3001, CYCLE_MIDDLE = 300, CYCLE_EDGE = 72, CYCLE_APART = 8, CYCLE_LAUNCHES = 10923;
static std::vector<uint16_t> cycle_frame(bool edge, uint32_t index) {
    uint32_t state = (index + 1u) * 2654435761u ^ (edge ? 0x5BD1E995u : 0u);
    std::vector<uint16_t> px(64);
    for (uint16_t &v : px) {
        state = state * 1664525u + 1013904223u;
        v = (uint16_t)(((state >> 8) & 15u) * (edge ? CYCLE_EDGE_STEP : 4096u));
    }
    return px;
}
static void whole_cycle() {
    constexpr uint32_t W = 8, H = 8;
    const uint32_t rows = dec16l_rows((uint64_t)W * H, 1);
    std::vector<std::vector<uint16_t>> px[2];
    std::vector<std::vector<uint8_t>> st[2];
    for (int edge = 0; edge < 2; edge++)
        for (uint32_t i = 0; i < (edge ? CYCLE_EDGE : CYCLE_MIDDLE); i++) {
            px[edge].push_back(cycle_frame(edge, i));
            st[edge].push_back(compress(px[edge].back(), W, H, 0, 1));
        }
    const std::unique_ptr<LaneQuad[]> tab(new LaneQuad[(size_t)rows * 4]);
    const std::unique_ptr<uint16_t[]> out(new uint16_t[W * H]);
    const auto at = [&](uint32_t) { return out.get(); };
    const auto decodes = [&](int edge, uint32_t i, uint32_t epoch) {
        const int rc = walk16<false, false, uint16_t>(st[edge][i].data(), st[edge][i].size(), W, H, 0, at, tab.get(), epoch);
        return rc == FELICS_OK && std::equal(px[edge][i].begin(), px[edge][i].end(), out.get());
    };
    const auto tagged = [&](uint32_t epoch) {
        unsigned long n = 0;
        for (uint32_t r = 0; r < rows; r++) n += (tab[(size_t)r * 4 + 3].w >> 17) == epoch;
        return n;
    };
    unsigned long wrong = 0, left = 0, wrong_plain = 0, left_plain = 0;
#if defined(__SANITIZE_ADDRESS__)
    constexpr uint32_t SLOTS = 8;  // (the sanitizer build: the same walks, fewer of them)
#else
    constexpr uint32_t SLOTS = 64;
#endif
    for (int plain = 0; plain < 2; plain++)  // plain: middle frames in every launch
        for (uint32_t slot = 0; slot < (plain ? 8u : SLOTS); slot++) {
            memset(tab.get(), 0, (size_t)rows * 4 * sizeof(LaneQuad));
            for (uint32_t launch = 1; launch < CYCLE_LAUNCHES; launch++) {
                const bool edge = !plain && launch == 1;
                const uint32_t frame = edge ? slot : ((launch - 1) * 64 + slot) % CYCLE_MIDDLE;
                if (!decodes(edge, frame, 1 + 3 * (launch - 1))) FAIL("whole cycle: slot %u launch %u on rows of other epochs", slot, launch);
            }
            const uint32_t last = plain ? ((CYCLE_LAUNCHES - 1) * 64 + slot) % CYCLE_MIDDLE : slot + CYCLE_APART;
            (plain ? left_plain : left) += tagged(1);
            (plain ? wrong_plain : wrong) += !decodes(!plain, last, 1);  // no clear: epoch 1 again
            memset(tab.get(), 0, (size_t)rows * 4 * sizeof(LaneQuad));
            if (!decodes(!plain, last, 1)) FAIL("whole cycle: slot %u launch %u behind a clear", slot, CYCLE_LAUNCHES);
        }
    printf("whole cycle: without the clear %lu of %u slots decode wrongly in launch %u (rows still tagged epoch 1 in front of it: %lu); "
           "middle frames in every launch: %lu of 8 (rows: %lu)\n", wrong, SLOTS, CYCLE_LAUNCHES, left, wrong_plain, left_plain);
    if (wrong * 2 < SLOTS) FAIL("whole cycle: fewer than half the slots notice the missing clear");
}

int main() {
    whole_planes();
    pitched();
    from_checkpoints();
    damage();
    stale_table();
    whole_cycle();
    printf("all checks held\n");
    return 0;
}
