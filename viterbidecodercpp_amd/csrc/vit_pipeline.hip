// vit_pipeline.hip -- vit_hip_pipeline_*: batches fed to the plan's update and chainback kernels from several streams, and the
// rules that pick the schedule.  No kernel of its own: the launches go through vit_hip.hip (vit_internal.hpp).
#include <new>

#include "vit_internal.hpp"

using namespace vit;

// the schedule of a pipeline, fixed at create time (pipeline_schedule below)
struct PipelineSchedule {
    int n_ws = 2, n_upd = 1;            // n_ws decision workspaces used round robin, n_upd update streams
    bool cb_small = false;              // K = 7 beside update waves: the 32-register LDS-ring chainback kernel
    size_t overlap_max_frames = 0;      // largest batch whose chainback is worth running beside the next update
    size_t two_updates_max_frames = 0;  // largest batch that leaves room for a second update kernel beside the first
    unsigned cb_wave_priority = 0;      // two-update schedule: the chainback kernel outranks the update waves
    size_t sub_frames = 0;              // a submitted batch is fed to the kernels in sub-batches of at most this many frames
};

struct vit_hip_pipeline : PipelineSchedule {
    vit_hip_handle h = nullptr;
    size_t max_frames = 0, L = 0, ws_bytes = 0;
    static constexpr int MAX_UPD = 3, MAX_WS = 4;
    void* ws[MAX_WS] = {nullptr, nullptr, nullptr, nullptr};
    hipStream_t s_upd[MAX_UPD] = {nullptr, nullptr, nullptr}, s_cb = nullptr;
    hipEvent_t upd_done[MAX_WS] = {nullptr, nullptr, nullptr, nullptr}, cb_done[MAX_WS] = {nullptr, nullptr, nullptr, nullptr};
    bool cb_pending[MAX_WS] = {false, false, false, false};
    unsigned long long n = 0;
    size_t last_first_frame = 0, last_frames = 0;   // frame range of the most recent sub-batch (the one ws[(n-1) % n_ws] holds)
    size_t sym_frame_bytes = 0, out_frame_bytes = 0;
    // optional per-batch timing (vit_hip_pipeline_set_timing): four events per submitted batch, resolved by sync()
    bool timing = false;
    struct Rec { hipEvent_t u0, u1, c0, c1; };
    std::vector<Rec> pending_recs;
    std::vector<hipEvent_t> event_pool;
    std::vector<float> t_update, t_chainback, t_complete;   // ms; t_complete: end of the batch's chainback since epoch
    hipEvent_t epoch = nullptr;          // start of the first timed batch's update
};

namespace {
hipEvent_t pipe_event(vit_hip_pipeline* p) {
    if (!p->event_pool.empty()) {
        hipEvent_t e = p->event_pool.back();
        p->event_pool.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    return e;
}

// The three schedule rules: from the handle's plan and kernels, the largest batch, the caller's options (-1 / 0: the rule decides)
// and the device's CU count to the schedule.
PipelineSchedule pipeline_schedule(vit_hip_handle h, size_t max_frames, const vit_hip_pipeline_options& opt, int cus) {
    PipelineSchedule s;
    const bool reg = h->plan == VIT_HIP_PLAN_REG;
    // one update wave per SIMD
    const size_t per_wave = (reg && cus > 0) ? (size_t)4 * (size_t)cus * (size_t)h->reg_code.tile : 0;
    // Rule 1 -- chainback beside the next update.  The overlap pays while the update waves leave a chainback wave its registers
    // (by the kernels' DESCRIPTORS, kernel_desc.hpp: 512 per SIMD) and LDS: PLAN_REG with at most two update waves per SIMD (three
    // at K = 7 with the 32-register LDS-ring chainback).  A larger batch fills the SIMDs by itself (K7 131072 frames: 8.70 ms
    // overlapped vs 8.10 ms back to back), and the PLAN_LDS update takes whole CUs: those batches run back to back on one stream.
    // PLAN_LDS2: wherever the update waves a CU's LDS admits leave the chainback's 24 registers on every SIMD (K = 11, 12, 14, 15:
    // four waves of at most 120 -- K15 4096 x 8192: 51.6 -> 50.3 ms per batch; K = 13: three of 144).
    // Rule 2 -- two updates in flight.  A batch of at most ONE update wave per SIMD (frames <= 4 x CUs x tile: the 32768-frame
    // share of BASELINE configs[3]) issues at the one-wave rate (5.27 cycles per packed instruction against 4.52 with two
    // waves, profiles/r2_dep_rate.txt): a second update stream and a third workspace put the next batch's update beside it
    // (hard8 32768 x 8192: 2.01 -> 1.87 ms per batch; HISTORY.md, round 3).
    s.overlap_max_frames = 2 * per_wave;
    s.two_updates_max_frames = per_wave;
    // THREE update waves per SIMD and a chainback wave beside them: only with the K = 7 LDS-ring chainback kernel (3 x 152 + 32
    // of 512 registers by the kernel descriptors; 98304 x 8192: 161 Gbit/s overlapped against 139 back to back)
    if (per_wave > 0 && h->K == 7 && reg_chainback_fits_beside_updates(h->reg_code, h->shift, 3, true)) s.overlap_max_frames = 3 * per_wave;
    // PLAN_LDS2 codes whose update kernel is capped at 120 registers: the 24-register chainback fits beside four of its waves
    if (h->plan == VIT_HIP_PLAN_LDS2 && lds2_chainback_fits(h)) s.overlap_max_frames = (size_t)-1;
    if (opt.chainback_overlap >= 0) s.overlap_max_frames = opt.chainback_overlap ? (size_t)-1 : 0;
    if (opt.update_streams == 1) s.two_updates_max_frames = 0;                        // never two updates in flight
    if (opt.update_streams >= 2) s.two_updates_max_frames = s.overlap_max_frames;    // wherever the chainback is overlapped
    // Rule 3 -- sub-batches.  Where two update waves leave no registers (or LDS) for a chainback wave (no built-in code since
    // round 5: LTE is capped at 240 registers, DAB's chainback ring is 12 KiB, CDMA 2000 fetches its branch metrics in sub-chunks;
    // a run-time compiled code may still land here), the chainback of a two-waves-per-SIMD batch cannot run beside the next update
    // at all: any batch of more than one wave per SIMD is fed to the kernels as sub-batches of one update wave per SIMD from the
    // two update streams (LTE 65536 x 8192, round 3: 118 - 120 -> 133 - 145 Gbit/s).
    s.sub_frames = max_frames;
    s.n_upd = max_frames <= s.two_updates_max_frames ? 2 : 1;
    if (reg && s.two_updates_max_frames > 0 && max_frames > s.two_updates_max_frames &&
        !reg_chainback_fits_beside_updates(h->reg_code, h->shift, 2, /* K = 7: the LDS-ring kernel is the one that runs there */ h->K == 7)) {
        s.sub_frames = s.two_updates_max_frames;
        s.n_upd = 2;
    }
    // (per_wave: one update wave per SIMD, whatever opt.update_streams did to two_updates_max_frames above)
    if (opt.sub_batches == 1 && per_wave > 0 && max_frames > per_wave) { s.sub_frames = per_wave; s.n_upd = 2; }
    if (opt.sub_batches == 0 && s.sub_frames < max_frames) { s.sub_frames = max_frames; s.n_upd = 1; }
    if (opt.update_streams == 3 && per_wave > 0 && s.sub_frames <= per_wave) s.n_upd = 3;   // three update kernels in flight
    s.n_ws = opt.workspaces ? opt.workspaces : s.n_upd + 1;
    // K = 7, chainback beside the update waves of ONE update kernel: the LDS-ring kernel (32 registers, 24 KiB of LDS) leaves
    // the update waves their SIMDs -- 65536 x 8192: 157 -> 160 Gbit/s over the register-ring kernel (160 registers), which stays
    // the kernel of a chainback that runs alone (7 % faster there) and of the two-update schedule (there it runs at the higher wave
    // priority and has to be FAST, not small: hard8 32768 x 8192 163 against 145 Gbit/s)
    s.cb_small = reg && h->K == 7 && s.n_upd == 1;
    if (opt.chainback_small_kernel >= 0) s.cb_small = opt.chainback_small_kernel == 1 && reg && h->K == 7;
    s.cb_wave_priority = s.n_upd > 1 ? 1u : 0u;
    if (opt.chainback_wave_priority >= 0) s.cb_wave_priority = (unsigned)opt.chainback_wave_priority;
    return s;
}
}  // namespace

extern "C" {

#ifdef VIT_HIP_EXPERIMENTS
// A/B builds only (make EXPERIMENTS=1; scripts/gpu_ab.sh): the environment fills whatever the caller's options left to the rules.
// The shipped library has no such switch: vit_hip_pipeline_create_ex is the supported override.
static void pipeline_options_from_env(vit_hip_pipeline_options* o) {
    auto flag = [](const char* name, int32_t* v, int32_t unset) {
        const char* e = getenv(name);
        if (e && *v == unset && (*e == '0' || *e == '1')) *v = *e - '0';
    };
    flag("VIT_HIP_PIPELINE_OVERLAP", &o->chainback_overlap, -1);
    flag("VIT_HIP_PIPELINE_SPLIT", &o->sub_batches, -1);
    flag("VIT_HIP_PIPELINE_CB_SMALL", &o->chainback_small_kernel, -1);
    flag("VIT_HIP_PIPELINE_CB_PRIO", &o->chainback_wave_priority, -1);
    if (const char* e = getenv("VIT_HIP_PIPELINE_UPDATES")) if (o->update_streams == 0 && *e >= '1' && *e <= '3') o->update_streams = *e - '0';
    if (const char* e = getenv("VIT_HIP_PIPELINE_WS")) if (o->workspaces == 0 && *e >= '2' && *e <= '4') o->workspaces = *e - '0';
}
#endif

static int vit_hip_pipeline_create_impl(vit_hip_handle h, size_t max_frames, size_t L, const vit_hip_pipeline_options* want,
                                        vit_hip_pipeline_t* out) {
    if (!h || !out || max_frames == 0) return fail(VIT_HIP_ERR_INVALID_ARG, "bad pipeline arguments");
    *out = nullptr;
    // the caller's options, read up to the size its build knows; anything beyond stays at "rule"
    vit_hip_pipeline_options opt{(uint32_t)sizeof(vit_hip_pipeline_options), -1, 0, -1, 0, -1, -1};
    if (want) {
        if (want->struct_size < 2 * sizeof(uint32_t)) return fail(VIT_HIP_ERR_INVALID_ARG, "vit_hip_pipeline_options.struct_size is not set");
        memcpy(&opt, want, want->struct_size < sizeof(opt) ? want->struct_size : sizeof(opt));
        if (opt.chainback_overlap < -1 || opt.chainback_overlap > 1 || opt.update_streams < 0 || opt.update_streams > 3 ||
            opt.sub_batches < -1 || opt.sub_batches > 1 || (opt.workspaces != 0 && (opt.workspaces < 2 || opt.workspaces > 4)) ||
            opt.chainback_small_kernel < -1 || opt.chainback_small_kernel > 1 || opt.chainback_wave_priority < -1 || opt.chainback_wave_priority > 1)
            return fail(VIT_HIP_ERR_INVALID_ARG, "vit_hip_pipeline_options: field out of range");
    }
#ifdef VIT_HIP_EXPERIMENTS
    pipeline_options_from_env(&opt);
#endif
    VIT_HIP_ON_DEVICE(h->device);
    vit_hip_pipeline* p = new (std::nothrow) vit_hip_pipeline();
    if (!p) return fail(VIT_HIP_ERR_RUNTIME, "out of host memory");
    p->h = h; p->max_frames = max_frames; p->L = L;
    int cus = 0;
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device);
    static_cast<PipelineSchedule&>(*p) = pipeline_schedule(h, max_frames, opt, cus);
    p->ws_bytes = vit_hip_workspace_bytes(h, p->sub_frames, L);
    p->sym_frame_bytes = (L + (size_t)h->K - 1) * (size_t)h->R * (size_t)h->soft_bytes;
    p->out_frame_bytes = (L + 7) / 8;
    int lo = 0, hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&lo, &hi);           // hi = numerically lowest = highest priority
    bool ok = hipStreamCreateWithPriority(&p->s_cb, hipStreamNonBlocking, hi) == hipSuccess;   // the short bit chase gets out of the update's way
    for (int k = 0; k < p->n_upd && ok; ++k) ok = hipStreamCreateWithFlags(&p->s_upd[k], hipStreamNonBlocking) == hipSuccess;
    for (int k = 0; k < p->n_ws && ok; ++k)
        ok = hipMalloc(&p->ws[k], p->ws_bytes) == hipSuccess &&
             hipEventCreateWithFlags(&p->upd_done[k], hipEventDisableTiming) == hipSuccess &&
             hipEventCreateWithFlags(&p->cb_done[k], hipEventDisableTiming) == hipSuccess;
    if (!ok) {
        (void)vit_hip_pipeline_destroy(p);
        return fail(VIT_HIP_ERR_RUNTIME, "pipeline allocation failed (two or three decision workspaces of vit_hip_workspace_bytes each)");
    }
    *out = p;
    return VIT_HIP_OK;
}

int vit_hip_pipeline_create(vit_hip_handle h, size_t max_frames, size_t L, vit_hip_pipeline_t* out) {
    VIT_HIP_NOTHROW(return vit_hip_pipeline_create_impl(h, max_frames, L, nullptr, out));
}

int vit_hip_pipeline_create_ex(vit_hip_handle h, size_t max_frames, size_t L, const vit_hip_pipeline_options* want,
                               vit_hip_pipeline_t* out) {
    VIT_HIP_NOTHROW(return vit_hip_pipeline_create_impl(h, max_frames, L, want, out));
}

static int vit_hip_pipeline_submit_impl(vit_hip_pipeline_t p, const void* d_symbols, size_t frames, uint8_t* d_bytes_out,
                            const uint32_t* d_end_state, void* done_event) {
    if (!p) return fail(VIT_HIP_ERR_INVALID_ARG, "NULL pipeline");
    if (frames > p->max_frames) return fail(VIT_HIP_ERR_INVALID_ARG, "batch larger than the pipeline was created for");
    if (frames == 0) return VIT_HIP_OK;
    VIT_HIP_ON_DEVICE(p->h->device);
    // a batch goes to the kernels in sub-batches of at most sub_frames frames (one, unless pipeline_create chose to split)
    for (size_t f0 = 0; f0 < frames; f0 += p->sub_frames) {
        const size_t nf = frames - f0 < p->sub_frames ? frames - f0 : p->sub_frames;
        const bool last = f0 + nf >= frames;
        const uint8_t* sym = (const uint8_t*)d_symbols + f0 * p->sym_frame_bytes;
        uint8_t* out = d_bytes_out + f0 * p->out_frame_bytes;
        const uint32_t* es = d_end_state ? d_end_state + f0 : nullptr;
        const int k = (int)(p->n % (unsigned long long)p->n_ws);
        hipStream_t s_upd = p->s_upd[(int)(p->n % (unsigned long long)p->n_upd)];
        vit_hip_pipeline::Rec rec{nullptr, nullptr, nullptr, nullptr};
        // the four timing events go back to the pool on every early exit (an error below leaves the sub-batches already
        // enqueued in flight: the caller syncs -- or destroys -- the pipeline before touching the buffers again)
        struct RecGuard {
            vit_hip_pipeline* p; vit_hip_pipeline::Rec* r; bool armed = true;
            ~RecGuard() {
                if (!armed) return;
                for (hipEvent_t e : {r->u0, r->u1, r->c0, r->c1})
                    if (e && e != p->epoch) p->event_pool.push_back(e);
            }
        } rec_guard{p, &rec};
        if (p->timing) {
            rec.u0 = pipe_event(p); rec.u1 = pipe_event(p); rec.c0 = pipe_event(p); rec.c1 = pipe_event(p);
            if (!rec.u0 || !rec.u1 || !rec.c0 || !rec.c1) return fail(VIT_HIP_ERR_RUNTIME, "hipEventCreate failed");
        }
        // the chainback that last read this workspace must have finished before the update overwrites it
        if (p->cb_pending[k]) VIT_HIP_CHECK(hipStreamWaitEvent(s_upd, p->cb_done[k], 0));
        if (p->timing) {
            VIT_HIP_CHECK(hipEventRecord(rec.u0, s_upd));
            if (!p->epoch) p->epoch = rec.u0;
        }
        int rc = vit_hip_update_batch(p->h, sym, nf, p->L + (size_t)p->h->K - 1, p->L, p->ws[k], p->ws_bytes, nullptr, nullptr, nullptr, s_upd);
        if (rc != VIT_HIP_OK) return rc;
        if (p->timing) VIT_HIP_CHECK(hipEventRecord(rec.u1, s_upd));
        hipStream_t s_cb = s_upd;                                   // back to back unless the overlap pays (pipeline_create)
        if (frames <= p->overlap_max_frames || p->n_upd > 1) {
            // all chainbacks go through ONE stream: batches complete in submit order whichever update stream fed them
            s_cb = p->s_cb;
            VIT_HIP_CHECK(hipEventRecord(p->upd_done[k], s_upd));
            VIT_HIP_CHECK(hipStreamWaitEvent(s_cb, p->upd_done[k], 0));
        }
        if (p->timing) VIT_HIP_CHECK(hipEventRecord(rec.c0, s_cb));
        rc = chainback_batch_impl(p->h, p->ws[k], nf, p->L, out, es, s_cb, p->cb_wave_priority, p->cb_small && s_cb != s_upd);
        if (rc != VIT_HIP_OK) return rc;
        if (p->timing) {
            VIT_HIP_CHECK(hipEventRecord(rec.c1, s_cb));
            p->pending_recs.push_back(rec);
        }
        rec_guard.armed = false;
        VIT_HIP_CHECK(hipEventRecord(p->cb_done[k], s_cb));
        if (done_event && last) VIT_HIP_CHECK(hipEventRecord((hipEvent_t)done_event, s_cb));
        p->cb_pending[k] = true;
        p->last_first_frame = f0;
        p->last_frames = nf;
        p->n++;
    }
    return VIT_HIP_OK;
}

int vit_hip_pipeline_submit(vit_hip_pipeline_t p, const void* d_symbols, size_t frames, uint8_t* d_bytes_out,
                            const uint32_t* d_end_state, void* done_event) {
    VIT_HIP_NOTHROW(return vit_hip_pipeline_submit_impl(p, d_symbols, frames, d_bytes_out, d_end_state, done_event));
}

static int vit_hip_pipeline_sync_impl(vit_hip_pipeline_t p) {
    if (!p) return fail(VIT_HIP_ERR_INVALID_ARG, "NULL pipeline");
    VIT_HIP_ON_DEVICE(p->h->device);
    for (int k = 0; k < p->n_upd; ++k) VIT_HIP_CHECK(hipStreamSynchronize(p->s_upd[k]));
    VIT_HIP_CHECK(hipStreamSynchronize(p->s_cb));
    // resolve the timing records of the batches that have now completed
    for (const auto& r : p->pending_recs) {
        float u = 0.f, c = 0.f, d = 0.f;
        VIT_HIP_CHECK(hipEventElapsedTime(&u, r.u0, r.u1));
        VIT_HIP_CHECK(hipEventElapsedTime(&c, r.c0, r.c1));
        VIT_HIP_CHECK(hipEventElapsedTime(&d, p->epoch, r.c1));
        p->t_update.push_back(u); p->t_chainback.push_back(c); p->t_complete.push_back(d);
    }
    for (const auto& r : p->pending_recs) {
        if (r.u0 != p->epoch) p->event_pool.push_back(r.u0);
        p->event_pool.push_back(r.u1); p->event_pool.push_back(r.c0); p->event_pool.push_back(r.c1);
    }
    p->pending_recs.clear();
    return VIT_HIP_OK;
}

int vit_hip_pipeline_sync(vit_hip_pipeline_t p) { VIT_HIP_NOTHROW(return vit_hip_pipeline_sync_impl(p)); }

static int vit_hip_pipeline_set_timing_impl(vit_hip_pipeline_t p, int enable) {
    if (!p) return fail(VIT_HIP_ERR_INVALID_ARG, "NULL pipeline");
    const int rc = vit_hip_pipeline_sync_impl(p);               // nothing in flight while the records are reset
    if (rc != VIT_HIP_OK) return rc;
    p->t_update.clear(); p->t_chainback.clear(); p->t_complete.clear();
    if (p->epoch) { p->event_pool.push_back(p->epoch); p->epoch = nullptr; }
    p->timing = enable != 0;
    return VIT_HIP_OK;
}

int vit_hip_pipeline_set_timing(vit_hip_pipeline_t p, int enable) { VIT_HIP_NOTHROW(return vit_hip_pipeline_set_timing_impl(p, enable)); }

int vit_hip_pipeline_get_timing(vit_hip_pipeline_t p, size_t capacity, float* update_ms, float* chainback_ms, float* complete_ms,
                                size_t* n_batches) {
    if (!p || !n_batches) return fail(VIT_HIP_ERR_INVALID_ARG, "NULL argument");
    const size_t n = p->t_update.size();
    *n_batches = n;
    for (size_t i = 0; i < n && i < capacity; ++i) {
        if (update_ms) update_ms[i] = p->t_update[i];
        if (chainback_ms) chainback_ms[i] = p->t_chainback[i];
        if (complete_ms) complete_ms[i] = p->t_complete[i];
    }
    return VIT_HIP_OK;
}

int vit_hip_pipeline_last_workspace(vit_hip_pipeline_t p, void** d_workspace, size_t* first_frame, size_t* frames) {
    if (!p || !d_workspace) return fail(VIT_HIP_ERR_INVALID_ARG, "NULL argument");
    if (p->n == 0) return fail(VIT_HIP_ERR_INVALID_ARG, "no batch has been submitted");
    *d_workspace = p->ws[(int)((p->n - 1) % (unsigned long long)p->n_ws)];
    if (first_frame) *first_frame = p->last_first_frame;
    if (frames) *frames = p->last_frames;
    return VIT_HIP_OK;
}

int vit_hip_pipeline_get_schedule_v2(vit_hip_pipeline_t p, vit_hip_pipeline_schedule* out, size_t schedule_bytes) {
    if (!p || !out) return fail(VIT_HIP_ERR_INVALID_ARG, "NULL argument");
    vit_hip_pipeline_schedule full;
    vit_hip_pipeline_schedule* s = &full;
    memset(s, 0, sizeof(*s));
    s->workspaces = p->n_ws;
    s->update_streams = p->n_upd;
    s->chainback_overlapped = (p->n_upd > 1 || p->max_frames <= p->overlap_max_frames) ? 1 : 0;
    s->overlap_max_frames = p->overlap_max_frames;
    s->two_updates_max_frames = p->two_updates_max_frames;
    s->workspace_bytes_each = p->ws_bytes;
    s->sub_batch_frames = p->sub_frames;
    s->chainback_wave_priority = (int32_t)p->cb_wave_priority;
    s->chainback_small_kernel = (p->cb_small && s->chainback_overlapped) ? 1 : 0;
    memcpy(out, s, schedule_bytes < sizeof(full) ? schedule_bytes : sizeof(full));
    return VIT_HIP_OK;
}

int vit_hip_pipeline_get_schedule(vit_hip_pipeline_t p, vit_hip_pipeline_schedule* s) {
    // the struct as binaries built against the header that introduced this symbol know it: it already ended in
    // chainback_small_kernel + reserved and this entry point filled them.  Fields added later are reached through _v2 only.
    return vit_hip_pipeline_get_schedule_v2(p, s, offsetof(vit_hip_pipeline_schedule, reserved) + sizeof(int32_t));
}

int vit_hip_pipeline_wait_event(vit_hip_pipeline_t p, void* event) {
    if (!p || !event) return fail(VIT_HIP_ERR_INVALID_ARG, "NULL argument");
    VIT_HIP_ON_DEVICE(p->h->device);
    // the next batch may go to any update stream (two-update schedules alternate): all of them wait
    for (int k = 0; k < p->n_upd; ++k) VIT_HIP_CHECK(hipStreamWaitEvent(p->s_upd[k], (hipEvent_t)event, 0));
    return VIT_HIP_OK;
}

int vit_hip_pipeline_destroy(vit_hip_pipeline_t p) {
    if (!p) return VIT_HIP_OK;
    DeviceGuard guard(p->h->device);
    for (int k = 0; k < vit_hip_pipeline::MAX_UPD; ++k)
        if (p->s_upd[k]) (void)hipStreamSynchronize(p->s_upd[k]);
    if (p->s_cb) (void)hipStreamSynchronize(p->s_cb);
    for (int k = 0; k < vit_hip_pipeline::MAX_WS; ++k) {
        if (p->ws[k]) (void)hipFree(p->ws[k]);
        if (p->upd_done[k]) (void)hipEventDestroy(p->upd_done[k]);
        if (p->cb_done[k]) (void)hipEventDestroy(p->cb_done[k]);
    }
    for (const auto& r : p->pending_recs) {
        if (r.u0 && r.u0 != p->epoch) (void)hipEventDestroy(r.u0);
        if (r.u1) (void)hipEventDestroy(r.u1);
        if (r.c0) (void)hipEventDestroy(r.c0);
        if (r.c1) (void)hipEventDestroy(r.c1);
    }
    if (p->epoch) (void)hipEventDestroy(p->epoch);
    for (hipEvent_t e : p->event_pool) (void)hipEventDestroy(e);
    for (int k = 0; k < vit_hip_pipeline::MAX_UPD; ++k)
        if (p->s_upd[k]) (void)hipStreamDestroy(p->s_upd[k]);
    if (p->s_cb) (void)hipStreamDestroy(p->s_cb);
    delete p;
    return VIT_HIP_OK;
}

}  // extern "C"
