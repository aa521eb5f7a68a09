// rt_render's device -> host copies: the copy stream, the SDMA engines driven directly, the
// row map of a tile (OutMap, rt_ctx.hpp), plain and sparse copies and their pinned buffers.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "rt_ctx.hpp"

namespace rtamd {

// The stream of rt_render's device -> host copies.  A CU-masked stream (mask = every CU) gets a
// hardware queue of its own (ensure_bstreams), so the copies never queue behind the render's launches.
int ensure_copy_stream(rt_ctx* c) {
    if (c->copy_stream) return RT_OK;
    std::vector<uint32_t> mask((c->n_cu + 31) / 32, 0u);
    for (int cu = 0; cu < c->n_cu; ++cu) mask[cu / 32] |= 1u << (cu % 32);
    if (hipExtStreamCreateWithCUMask(&c->copy_stream, static_cast<uint32_t>(mask.size()), mask.data()) != hipSuccess) {
        (void)hipGetLastError();
        HIP_TRY(c, hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
    }
    return RT_OK;
}

// Device buffers of the sparse host copies for a tw x rows tile (segment bits, row counts, row
// offsets, and the packed BGR / RGB sections of the outputs requested at their largest: every
// segment flagged), grown on demand.  They are not part of the working-set budget, so they are
// taken only from what the device has free beyond kRuntimeHeadroom; if they do not fit (or
// hipMalloc fails) *ok is false and the render copies its frame the plain way.
int ensure_sparse(rt_ctx* c, hipStream_t st, uint32_t tw, uint32_t rows, bool bgr, bool rgb, bool* ok) {
    *ok = false;
    int rc = ensure_copy_stream(c);
    if (rc != RT_OK) return rc;
    if (!c->sp_cam) HIP_TRY(c, hipEventCreateWithFlags(&c->sp_cam, hipEventDisableTiming));
    if (!c->sp_ready) HIP_TRY(c, hipEventCreateWithFlags(&c->sp_ready, hipEventDisableTiming));
    const uint64_t nseg = (tw + kSegPx - 1) / kSegPx, words = (nseg + 31) / 32, segs = nseg * rows;
    const uint64_t s_bits = align_up(rows * words * 4, 256), s_cnt = align_up(rows * 4ull, 256),
                   s_off = align_up((rows + 1ull) * 4, 256), s_bgr = bgr ? align_up(segs * 3 * kSegPx, 256) : 0,
                   s_rgb = rgb ? segs * 3 * kSegPx * sizeof(float) : 0;
    const uint64_t need = s_bits + s_cnt + s_off + s_bgr + s_rgb;
    if (need > c->sp_cap) {
        HIP_TRY(c, hipStreamSynchronize(st));
        HIP_TRY(c, hipStreamSynchronize(c->copy_stream));
        if (c->d_sp) (void)hipFree(c->d_sp);
        c->d_sp = nullptr;
        c->sp_cap = 0;
        size_t fr = 0, total = 0;
        if (hipMemGetInfo(&fr, &total) != hipSuccess) { (void)hipGetLastError(); return RT_OK; }
        if (need > fr || fr - need < kRuntimeHeadroom) return RT_OK;
        if (hipMalloc(&c->d_sp, need) != hipSuccess) {
            (void)hipGetLastError();
            c->d_sp = nullptr;
            return RT_OK;
        }
        c->sp_cap = need;
    }
    auto* base = static_cast<uint8_t*>(c->d_sp);
    c->d_sp_bits = reinterpret_cast<uint32_t*>(base);
    c->d_sp_cnt = reinterpret_cast<uint32_t*>(base + s_bits);
    c->d_sp_off = reinterpret_cast<uint32_t*>(base + s_bits + s_cnt);
    c->d_sp_bgr = bgr ? base + s_bits + s_cnt + s_off : nullptr;
    c->d_sp_rgb = rgb ? reinterpret_cast<float*>(base + s_bits + s_cnt + s_off + s_bgr) : nullptr;
    *ok = true;
    return RT_OK;
}

// ---- SDMA copy engines (tuning copy_engine) --------------------------------------------
// hipMemcpyAsync moves rt_render's frame to the host at ~29 GB/s on the boxes measured
// (tools/sdma_probe.hip: a blit kernel or the runtime's choice of engine), one SDMA engine
// driven directly at ~53 GB/s.  The engine's queue does not see HIP events, so the host waits
// for the event a copy depends on (hipEventSynchronize) before it queues the copy; each batch
// of copies completes a signal the host waits on.
static hsa_status_t sdma_find_agents(hsa_agent_t a, void* data) {
    auto* c = static_cast<rt_ctx*>(data);
    hsa_device_type_t t;
    if (hsa_agent_get_info(a, HSA_AGENT_INFO_DEVICE, &t) != HSA_STATUS_SUCCESS) return HSA_STATUS_SUCCESS;
    if (t == HSA_DEVICE_TYPE_CPU && c->hsa_cpu.handle == 0) c->hsa_cpu = a;
    if (t == HSA_DEVICE_TYPE_GPU && c->hsa_gpu.handle == 0) {
        // the HIP device's agent: same PCI domain, bus and device
        uint32_t bdf = 0, dom = 0;
        int bus = -1, dev = -1, hdom = -1;
        (void)hsa_agent_get_info(a, static_cast<hsa_agent_info_t>(HSA_AMD_AGENT_INFO_BDFID), &bdf);
        (void)hsa_agent_get_info(a, static_cast<hsa_agent_info_t>(HSA_AMD_AGENT_INFO_DOMAIN), &dom);
        if (hipDeviceGetAttribute(&bus, hipDeviceAttributePciBusId, c->device) == hipSuccess &&
            hipDeviceGetAttribute(&dev, hipDeviceAttributePciDeviceId, c->device) == hipSuccess &&
            hipDeviceGetAttribute(&hdom, hipDeviceAttributePciDomainID, c->device) == hipSuccess &&
            static_cast<int>((bdf >> 8) & 0xFF) == bus && static_cast<int>((bdf >> 3) & 0x1F) == dev &&
            static_cast<int>(dom) == hdom)
            c->hsa_gpu = a;
        (void)hipGetLastError();
    }
    return HSA_STATUS_SUCCESS;
}

// Set up once per context; false if the device has no usable engine (the HIP path is used).
static bool sdma_setup(rt_ctx* c) {
    if (c->sdma_state) return c->sdma_state == 1;
    c->sdma_state = -1;
    if (hsa_init() != HSA_STATUS_SUCCESS) return false;
    bool ok = hsa_iterate_agents(sdma_find_agents, c) == HSA_STATUS_SUCCESS && c->hsa_gpu.handle && c->hsa_cpu.handle &&
              hsa_amd_memory_copy_engine_status(c->hsa_cpu, c->hsa_gpu, &c->sdma_avail) == HSA_STATUS_SUCCESS &&
              c->sdma_avail != 0;
    if (ok && hsa_amd_memory_get_preferred_copy_engine(c->hsa_cpu, c->hsa_gpu, &c->sdma_pref) != HSA_STATUS_SUCCESS)
        c->sdma_pref = 0;
    for (int i = 0; ok && i < rt_ctx::kSdmaSignals; ++i) ok = hsa_signal_create(0, 0, nullptr, &c->sdma_sig[i]) == HSA_STATUS_SUCCESS;
    if (!ok) {
        for (hsa_signal_t& sg : c->sdma_sig)
            if (sg.handle) { (void)hsa_signal_destroy(sg); sg.handle = 0; }
        (void)hsa_shut_down();
        return false;
    }
    c->sdma_state = 1;
    return true;
}

// The engines rt_render's copies use now, as a mask taken in turn (0: hipMemcpyAsync).  -1: the
// device's engines 0-3 (tools/sdma_probe: ~53 GB/s each on MI355X, the PCIe link's rate; engines
// 4-15 move 7-12.5 GB/s); several in turn hide each copy's fixed cost behind the others' transfers
// (a rank's 64 row bands of 192 KB: 38 GB/s on four engines, 14 GB/s on one).
uint32_t sdma_engine(rt_ctx* c, RenderReq req) {
    int64_t e = c->t(kTuneCopyEngine);
    if (e == -2) e = req.banded_copy ? -1 : 0;
    if (e == 0 || !sdma_setup(c)) return 0;
    if (e > 0) return (1u << (e - 1)) & c->sdma_avail;
    if (c->sdma_avail & 0xFu) return c->sdma_avail & 0xFu;
    const uint32_t m = (c->sdma_pref & c->sdma_avail) ? (c->sdma_pref & c->sdma_avail) : c->sdma_avail;
    return m & (~m + 1u);
}

// Wait until signal `si` is 0 (every copy counted on it done); a copy that has not completed
// after 30 s is an error, not a hang.
int sdma_wait(rt_ctx* c, int si) {
    static const uint64_t hint = [] {
        uint64_t f = 0;
        return hsa_system_get_info(HSA_SYSTEM_INFO_TIMESTAMP_FREQUENCY, &f) == HSA_STATUS_SUCCESS && f ? f / 1000 : 1000000;
    }();
    const auto t0 = std::chrono::steady_clock::now();
    while (hsa_signal_wait_scacquire(c->sdma_sig[si], HSA_SIGNAL_CONDITION_EQ, 0, hint, HSA_WAIT_STATE_ACTIVE) != 0)
        if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(30))
            return fail(c, RT_E_HIP, "an SDMA copy did not complete");
    return RT_OK;
}

// Device -> pinned host copy on the next engine of `engines` (in turn), counted on signal `si` (one
// more pending copy); the caller waits with sdma_wait.  Copies on different engines complete in
// any order: a wait covers exactly the copies counted on its signal.
int sdma_copy(rt_ctx* c, uint32_t engines, int si, void* dst, const void* src, size_t bytes) {
    if (!bytes) return RT_OK;
    uint32_t engine = 0;
    for (int k = 0; k < 32 && !engine; ++k) {
        const uint32_t bit = 1u << (c->sdma_turn++ & 31u);
        if (engines & bit) engine = bit;
    }
    hsa_signal_t sg = c->sdma_sig[si];
    hsa_signal_add_screlease(sg, 1);
    const hsa_status_t st = hsa_amd_memory_async_copy_on_engine(dst, c->hsa_cpu, src, c->hsa_gpu, bytes, 0, nullptr, sg,
                                                                static_cast<hsa_amd_sdma_engine_id_t>(engine), true);
    if (st != HSA_STATUS_SUCCESS) {
        hsa_signal_subtract_screlease(sg, 1);
        (void)sdma_wait(c, si);              // the copies queued before it still complete
        return fail(c, RT_E_HIP, "hsa_amd_memory_async_copy_on_engine failed (" + std::to_string(st) + ")");
    }
    return RT_OK;
}

// Wait for an event by polling it: a blocking wait's wake-up costs tens of microseconds, which a
// frame of a few hundred microseconds notices at every step of its copies.
static hipError_t spin_wait(hipEvent_t ev) {
    for (;;) {
        const hipError_t e = hipEventQuery(ev);
        if (e != hipErrorNotReady) return e;
        std::this_thread::yield();
    }
}

// Device -> caller-owned host memory, row band by row band: the copy stream
// waits for each band's fold (c->band_ev, recorded by the render when
// RenderReq::bands was set; otherwise for the whole render), so the PCIe transfer
// of the first bands overlaps the fold of the later ones.  A page-locked
// destination gets the DMA directly (one copy per run of rows that are
// consecutive on the host, 2D when the rows are not back to back); pageable
// memory goes through kRing pinned slices of whole rows, the copy engine
// filling slices ahead while the host pool empties them in order into their
// host rows.  wait = false (sparse copies): no wait on the bands, the copy
// stream's order alone (its segment kernels follow the camera pass).
int copy_to_host(rt_ctx* c, RenderReq req, void* dst, const void* src, const OutMap& m, uint32_t rows, hipEvent_t after,
                 bool sync) {
    if (!rows || !m.row_bytes) return RT_OK;
    int rc = ensure_copy_stream(c);
    if (rc != RT_OK) return rc;
    if (!c->cp_done) HIP_TRY(c, hipEventCreateWithFlags(&c->cp_done, hipEventDisableTiming));
    const uint32_t engine = sdma_engine(c, req);     // 0: hipMemcpyAsync on the copy stream
    const auto* s8 = static_cast<const uint8_t*>(src);
    auto* d8 = static_cast<uint8_t*>(dst);
    hipPointerAttribute_t attr{};
    const bool pinned = hipPointerGetAttributes(&attr, dst) == hipSuccess && attr.type == hipMemoryTypeHost;
    (void)hipGetLastError();                       // a pageable pointer is not an error
    const bool contig = m.contiguous();
    // pieces: rows [j0, j0 + n) of one chunk band, consecutive on the host (pinned), at most one
    // staging slice of rows (pageable)
    const size_t slice = std::max(kSlice, m.dev_pitch);
    const uint32_t slice_rows = static_cast<uint32_t>(std::max<size_t>(1, slice / m.dev_pitch));
    struct Piece { uint32_t j0, n; int band; };
    std::vector<Piece> pieces;
    const int nb = c->n_bands > 0 ? c->n_bands : 1;
    for (int bi = 0; bi < nb; ++bi) {
        const uint32_t a = c->n_bands > 0 ? c->band_row0[bi] : 0;
        const uint32_t e = c->n_bands > 0 ? std::min(rows, c->band_row0[bi] + c->band_nrows[bi]) : rows;
        for (uint32_t j = a; j < e;) {
            uint32_t n = 1;
            if (pinned) {
                while (j + n < e && m.next_row(j + n - 1) && (contig || n < 65535)) ++n;
            } else {
                n = std::min(slice_rows, e - j);
            }
            pieces.push_back(Piece{j, n, bi});
            j += n;
        }
    }
    // a piece is copied once its chunk band is final (band_ev; the whole render: render_done),
    // or after `after`: the copy stream waits for the event, the host for an engine's copies
    auto band_event = [&](int bi) { return after ? after : c->n_bands > 0 ? c->band_ev[bi] : c->render_done; };
    auto wait_band = [&](int bi) -> hipError_t {
        return engine ? hipEventSynchronize(band_event(bi)) : hipStreamWaitEvent(c->copy_stream, band_event(bi), 0);
    };
    // page-locked destination: every piece straight into the caller's rows, one copy per piece (the
    // rows of a partial-width tile: one per row), on the engines or the copy stream.  (Not
    // hipMemcpy2DAsync: a 2D copy of rows whose length is not a multiple of 4 was seen to land
    // after the stream's later event, tools/copy_stress.py.)
    if (pinned) {
        constexpr int si = rt_ctx::kSdmaSignals - 1;
        int last = -1;
        for (const Piece& pc : pieces) {
            if (pc.band != last) { HIP_TRY(c, wait_band(pc.band)); last = pc.band; }
            for (uint32_t j = pc.j0; j < pc.j0 + pc.n; j += contig ? pc.n : 1) {
                void* to = d8 + m.host_off(j);
                const void* from = s8 + j * m.dev_pitch;
                const size_t len = contig ? pc.n * m.dev_pitch : m.row_bytes;
                if (engine) {
                    if ((rc = sdma_copy(c, engine, si, to, from, len)) != RT_OK) return rc;
                } else {
                    HIP_TRY(c, hipMemcpyAsync(to, from, len, hipMemcpyDeviceToHost, c->copy_stream));
                }
            }
        }
        if (!sync) return RT_OK;
        if (engine) return sdma_wait(c, si);
        HIP_TRY(c, hipEventRecord(c->cp_done, c->copy_stream));
        HIP_TRY(c, spin_wait(c->cp_done));
        return RT_OK;
    }
    if (slice > c->pin_cap) {                      // rows wider than a slice: larger slices
        for (int i = 0; i < kRing; ++i) {
            if (c->pin[i]) (void)hipHostFree(c->pin[i]);
            c->pin[i] = nullptr;
        }
        c->pin_cap = slice;
    }
    for (int i = 0; i < kRing; ++i) {
        if (!c->pin[i]) HIP_TRY(c, hipHostMalloc(&c->pin[i], c->pin_cap, hipHostMallocDefault));
        if (!c->pin_ev[i]) HIP_TRY(c, hipEventCreateWithFlags(&c->pin_ev[i], hipEventDisableTiming));
    }
    const size_t n = pieces.size();
    size_t issued = 0, drained = 0;
    int last = -1;
    while (drained < n) {
        while (issued < n && issued - drained < static_cast<size_t>(kRing)) {   // slot issued % kRing is free
            const Piece& pc = pieces[issued];
            if (pc.band != last) { HIP_TRY(c, wait_band(pc.band)); last = pc.band; }
            const int slot = static_cast<int>(issued % kRing);
            if (engine) {
                if ((rc = sdma_copy(c, engine, slot, c->pin[slot], s8 + pc.j0 * m.dev_pitch, pc.n * m.dev_pitch)) != RT_OK)
                    return rc;
            } else {
                HIP_TRY(c, hipMemcpyAsync(c->pin[slot], s8 + pc.j0 * m.dev_pitch, pc.n * m.dev_pitch, hipMemcpyDeviceToHost,
                                          c->copy_stream));
                HIP_TRY(c, hipEventRecord(c->pin_ev[slot], c->copy_stream));
            }
            ++issued;
        }
        const int slot = static_cast<int>(drained % kRing);
        if (engine) {
            if ((rc = sdma_wait(c, slot)) != RT_OK) return rc;
        } else {
            HIP_TRY(c, spin_wait(c->pin_ev[slot]));
        }
        const Piece& pc = pieces[drained];
        const auto* from = static_cast<const uint8_t*>(c->pin[slot]);
        if (!m.frame && contig) {
            c->pool.copy(d8 + m.host_off(pc.j0), from, pc.n * m.dev_pitch);
        } else {                                   // row by row into the host rows, shared by the pool
            const size_t parts = std::min<size_t>(HostCopyPool::kParts, pc.n);
            c->pool.run(parts, [&](size_t q) {
                const uint32_t a = pc.j0 + static_cast<uint32_t>(pc.n * q / parts), e = pc.j0 + static_cast<uint32_t>(pc.n * (q + 1) / parts);
                for (uint32_t j = a; j < e; ++j) std::memcpy(d8 + m.host_off(j), from + (j - pc.j0) * m.dev_pitch, m.row_bytes);
            });
        }
        ++drained;
    }
    return RT_OK;
}

// Pinned host buffer of at least `bytes` (grown on demand).
int ensure_pinned(rt_ctx* c, void*& p, size_t& cap, size_t bytes) {
    if (bytes <= cap) return RT_OK;
    if (p) (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
    HIP_TRY(c, hipHostMalloc(&p, bytes, hipHostMallocDefault));
    cap = bytes;
    return RT_OK;
}

// rt_render's copies after a sparse render: the row offsets and segment bits,
// then the whole frame as the camera pass left it (every pixel without a chain is final; the
// generations run meanwhile), then, once the render is done, the packed chain segments in row
// ranges, each scattered into the host rows by the host pool as soon as it has landed.
int copy_sparse(rt_ctx* c, RenderReq req, const rt_render_opts* o, float* out_rgb, uint8_t* out_bgr, const OutMap& mr,
                const OutMap& mb) {
    const uint32_t rows = o->tile_h, tw = o->tile_w;
    const uint32_t nseg = (tw + kSegPx - 1) / kSegPx, words = (nseg + 31) / 32;
    const size_t s_off = (rows + 1ull) * 4, s_bits = static_cast<size_t>(rows) * words * 4;
    using Clock = std::chrono::steady_clock;
    const auto t0 = Clock::now();
    auto us = [&] { return std::chrono::duration<double, std::micro>(Clock::now() - t0).count(); };
    int rc = ensure_pinned(c, c->h_sp_meta, c->h_sp_meta_cap, s_off + s_bits);
    if (rc != RT_OK) return rc;
    auto* h_off = static_cast<uint32_t*>(c->h_sp_meta);
    auto* h_bits = h_off + (rows + 1);
    HIP_TRY(c, hipMemcpyAsync(h_off, c->d_sp_off, s_off, hipMemcpyDeviceToHost, c->copy_stream));
    HIP_TRY(c, hipMemcpyAsync(h_bits, c->d_sp_bits, s_bits, hipMemcpyDeviceToHost, c->copy_stream));
    if (!c->cp_done) HIP_TRY(c, hipEventCreateWithFlags(&c->cp_done, hipEventDisableTiming));
    HIP_TRY(c, hipEventRecord(c->cp_done, c->copy_stream));          // the offsets and bits have landed
    // the frame as the camera pass left it (sp_ready: after the segment kernels, which follow the camera pass):
    // into a page-locked frame the copies are only queued here (the packed ranges queue behind them and
    // the host waits for those), into pageable memory the staging slices are drained as they land
    const uint32_t engine = sdma_engine(c, req);
    if (out_bgr && (rc = copy_to_host(c, req, out_bgr, c->d_bgr, mb, rows, c->sp_ready, false)) != RT_OK) return rc;
    if (out_rgb && (rc = copy_to_host(c, req, out_rgb, c->d_rgb, mr, rows, c->sp_ready, false)) != RT_OK) return rc;
    const double t_queued = us();
    HIP_TRY(c, spin_wait(c->cp_done));
    const double t_frame = us();
    const uint64_t total = h_off[rows];
    const size_t seg_b = 3 * kSegPx, seg_r = 3 * kSegPx * sizeof(float);
    const size_t pk_b = out_bgr ? total * seg_b : 0, pk_r = out_rgb ? total * seg_r : 0;
    if ((rc = ensure_pinned(c, c->h_sp_pk, c->h_sp_pk_cap, std::max<size_t>(1, pk_b + pk_r))) != RT_OK) return rc;
    auto* hb = static_cast<uint8_t*>(c->h_sp_pk);
    auto* hr = reinterpret_cast<float*>(hb + pk_b);
    // the packed segments once the render is done: on the copy stream after its end event, or on the
    // engine once the host has seen it, in row ranges, each with its own event / signal
    const hipEvent_t done = c->n_bands > 0 ? c->band_ev[0] : c->render_done;
    if (engine) HIP_TRY(c, spin_wait(done));
    else HIP_TRY(c, hipStreamWaitEvent(c->copy_stream, done, 0));
    const double t_done = us();
    // ranges of at least ~2 MB (each copy has a fixed cost of its own), at most kSpRanges
    const int nr = static_cast<int>(std::max<uint64_t>(1, std::min<uint64_t>({static_cast<uint64_t>(rt_ctx::kSpRanges), rows,
                                                                             (pk_b + pk_r + (2u << 20) - 1) / (2u << 20)})));
    auto r_at = [&](int j) { return static_cast<uint32_t>(static_cast<uint64_t>(rows) * j / nr); };
    for (int j = 0; j < nr; ++j) {
        const uint64_t a = h_off[r_at(j)], e = h_off[r_at(j + 1)];
        if (engine) {
            if (e > a && out_bgr && (rc = sdma_copy(c, engine, kRing + j, hb + a * seg_b, c->d_sp_bgr + a * seg_b, (e - a) * seg_b)) != RT_OK)
                return rc;
            if (e > a && out_rgb &&
                (rc = sdma_copy(c, engine, kRing + j, hr + a * 3 * kSegPx, c->d_sp_rgb + a * 3 * kSegPx, (e - a) * seg_r)) != RT_OK)
                return rc;
            continue;
        }
        if (!c->sp_ev[j]) HIP_TRY(c, hipEventCreateWithFlags(&c->sp_ev[j], hipEventDisableTiming));
        if (e > a && out_bgr)
            HIP_TRY(c, hipMemcpyAsync(hb + a * seg_b, c->d_sp_bgr + a * seg_b, (e - a) * seg_b, hipMemcpyDeviceToHost, c->copy_stream));
        if (e > a && out_rgb)
            HIP_TRY(c, hipMemcpyAsync(hr + a * 3 * kSegPx, c->d_sp_rgb + a * 3 * kSegPx, (e - a) * seg_r, hipMemcpyDeviceToHost,
                                      c->copy_stream));
        HIP_TRY(c, hipEventRecord(c->sp_ev[j], c->copy_stream));
    }
    const size_t pad = mb.row_bytes - 3ull * tw;           // BMP row padding of the tile's rows (device pitch)
    auto* rgb8 = reinterpret_cast<uint8_t*>(out_rgb);
    auto scatter_rows = [&](uint32_t r0, uint32_t r1) {
        for (uint32_t r = r0; r < r1; ++r) {
            const uint32_t* bits = h_bits + static_cast<size_t>(r) * words;
            uint64_t i = h_off[r];
            for (uint32_t w = 0; w < words; ++w)
                for (uint32_t m = bits[w]; m; m &= m - 1, ++i) {
                    const uint32_t x0 = (w * 32 + static_cast<uint32_t>(__builtin_ctz(m))) * kSegPx;
                    const uint32_t n = std::min(kSegPx, tw - x0);
                    if (out_bgr) {
                        uint8_t* d = out_bgr + mb.host_off(r) + 3ull * x0;
                        std::memcpy(d, hb + i * seg_b, 3ull * n);
                        if (x0 + n == tw && pad) std::memset(d + 3ull * n, 0, pad);   // BMP row padding
                    }
                    if (out_rgb) std::memcpy(rgb8 + mr.host_off(r) + 12ull * x0, hr + i * 3 * kSegPx, 12ull * n);
                }
        }
    };
    // each range scattered by the pool as soon as it has landed (the later ones still in flight)
    double t_first = 0.0;
    // (engine: the frame's copies were queued on the same engine before the ranges; its signal first)
    if (engine && (rc = sdma_wait(c, rt_ctx::kSdmaSignals - 1)) != RT_OK) return rc;
    for (int j = 0; j < nr; ++j) {
        if (engine) {
            if ((rc = sdma_wait(c, kRing + j)) != RT_OK) return rc;
        } else {
            HIP_TRY(c, spin_wait(c->sp_ev[j]));
        }
        if (j == 0) t_first = us();
        const uint32_t ra = r_at(j), rb = r_at(j + 1);
        const size_t parts = std::min<size_t>(HostCopyPool::kParts, rb - ra);
        c->pool.run(parts, [&](size_t q) {
            scatter_rows(ra + static_cast<uint32_t>((rb - ra) * q / parts), ra + static_cast<uint32_t>((rb - ra) * (q + 1) / parts));
        });
    }
    if (c->t(kTuneVerbose))
        std::fprintf(stderr, "rtamd: sparse copy: %llu of %llu segments; frame copies queued at %.0f us, offsets in at %.0f, "
                     "render done seen at %.0f (engine only), first packed range in at %.0f, done at %.0f\n",
                     static_cast<unsigned long long>(total), static_cast<unsigned long long>(nseg) * rows, t_queued, t_frame,
                     engine ? t_done : 0.0, t_first, us());
    return RT_OK;
}

// rt_render's layout on both sides (check_opts has validated o): the device frame of the tile
// (f32 rows of 12 tile_w bytes, BGR rows of *dev_bgr_pitch bytes) and where each row goes on the host.
int host_layout(rt_ctx* c, const rt_render_opts* o, uint32_t pitch, OutMap& mr, OutMap& mb, uint32_t* dev_bgr_pitch) {
    const bool frame = (o->flags & RT_OUT_FRAME_ROWS) != 0;
    mr = OutMap{};
    mr.dev_pitch = mr.row_bytes = static_cast<size_t>(o->tile_w) * 12;
    mr.host_pitch = mr.dev_pitch;
    if (frame) {
        const uint32_t hp = o->bgr_pitch ? o->bgr_pitch : 3 * o->width;
        if (hp < 3ull * o->width) return fail(c, RT_E_INVALID, "RT_OUT_FRAME_ROWS: bgr_pitch < 3*width");
        mr.frame = true;
        mr.y0 = o->y0; mr.band = o->band ? o->band : 1; mr.stride = o->band_stride ? o->band_stride : 1; mr.phase = o->band_phase;
        mr.host_pitch = static_cast<size_t>(o->width) * 12;
        mr.host_x = static_cast<size_t>(o->x0) * 12;
        mb = mr;
        // the tile's BGR rows carry the frame's row padding when the tile ends at the frame's right edge
        const uint32_t pad = o->x0 + o->tile_w == o->width ? hp - 3 * o->width : 0;
        mb.dev_pitch = mb.row_bytes = 3ull * o->tile_w + pad;
        mb.host_pitch = hp;
        mb.host_x = 3ull * o->x0;
        *dev_bgr_pitch = 3 * o->tile_w + pad;
    } else {
        mb = OutMap{};
        mb.dev_pitch = mb.row_bytes = mb.host_pitch = pitch;
        *dev_bgr_pitch = pitch;
    }
    return RT_OK;
}

// rt_render's device frame for the tile: grown on demand (an earlier render may still write it).
int ensure_host_frame(rt_ctx* c, size_t rgb_bytes, size_t bgr_bytes) {
    if (c->render_pending && (rgb_bytes > c->rgb_cap || bgr_bytes > c->bgr_cap))
        HIP_TRY(c, hipEventSynchronize(c->render_done));
    if (rgb_bytes > c->rgb_cap) {
        if (c->d_rgb) (void)hipFree(c->d_rgb);
        c->d_rgb = nullptr; c->rgb_cap = 0;
        HIP_TRY(c, hipMalloc(&c->d_rgb, rgb_bytes));
        c->rgb_cap = rgb_bytes;
    }
    if (bgr_bytes > c->bgr_cap) {
        if (c->d_bgr) (void)hipFree(c->d_bgr);
        c->d_bgr = nullptr; c->bgr_cap = 0;
        HIP_TRY(c, hipMalloc(&c->d_bgr, bgr_bytes));
        c->bgr_cap = bgr_bytes;
    }
    return RT_OK;
}

}  // namespace rtamd
