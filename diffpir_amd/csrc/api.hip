// C ABI (include/diffpir_engine.h): lifecycle, memory plumbing, operator entry points and the
// restoration loops.  Each entry cites the reference interface it replaces in
// the header; this file only validates, dispatches to the launchers and keeps the error string.
// The whole-loop entries share one skeleton ("whole loop" below): loop_prologue -> film_table / loop_init -> run_steps (the one
// step driver with hipGraph capture; the gradient loops run an eager body instead) -> loop_finish.
#include "engine.h"
#include "grad.h"
#include "blur.h"
#include "inpaint.h"
#include "ancestral.h"
#include "progress.h"
#include "lpips.h"
#include "fid.h"
#include "metrics8.h"
#include "results.h"
#include <math.h>
#include <string.h>
#include <stdlib.h>

using namespace dpir;

static int fail(dpir_engine* e, const Status& s) {
    if (e) e->last_error = s.msg;
    return s.code;
}
#define API_TRY(e, expr)                          \
    do {                                          \
        Status _s = (expr);                       \
        if (!_s.ok()) return fail((e), _s);       \
    } while (0)
#define API_HIP(e, expr)                                                                  \
    do {                                                                                  \
        hipError_t _h = (expr);                                                           \
        if (_h != hipSuccess)                                                             \
            return fail((e), Status{DPIR_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_h)}); \
    } while (0)

// f16x3 operand range guard: called where the ABI synchronises anyway (dpir_sync, D2H copies).  A non-zero count means
// at least that many wave-lanes clamped an activation to the f16 range since the last check: the images are wrong.
// The failure is STICKY: every later dpir_sync / dpir_d2h / dpir_allgather_results keeps returning DPIR_ERR_RANGE (the device
// results stay wrong) until the next UNet forward or restoration loop starts (range_clear).
// Fused-hop time-out (bit 40 and up of the guard word): degrade, do not die.  Latches the hop off for this engine (the captured step graphs
// hold its kernels: dropped), clears the guard word and says so once on stderr.  Returns true when a time-out was seen.
static bool fuse_timeout_latch(dpir_engine* e, unsigned long long n) {
    if (n < (1ull << 40)) return false;
    e->fuse_h1_off = true;
    e->invalidate_graphs();
    (void)hipMemsetAsync(e->range_ctr, 0, sizeof(unsigned long long), e->stream);
    (void)hipStreamSynchronize(e->stream);
    fprintf(stderr, "diffpir: conv7's fused GroupNorm hop timed out (a workgroup waited too long for the other workgroups of its image: the GPU is shared "
                    "with other engines or processes).  The hop is switched off for this engine (unfused path from here on, ~2 %% slower) and the "
                    "affected work is re-run.\n");
    return true;
}
static int read_range(dpir_engine* e, unsigned long long* n) {
    *n = 0;
    if (hipMemcpyAsync(n, e->range_ctr, sizeof(*n), hipMemcpyDeviceToHost, e->stream) != hipSuccess ||
        hipStreamSynchronize(e->stream) != hipSuccess)
        return fail(e, Status{DPIR_ERR_HIP, "reading the operand range counter failed"});
    return DPIR_OK;
}
int dpir_check_range(dpir_engine* e) {
    if (!e->range_ctr || e->precision == 0) { e->fwd_since_sync = 0; e->replay_last = nullptr; return DPIR_OK; }
    unsigned long long n = 0;
    if (int rc = read_range(e, &n)) return rc;
    if (fuse_timeout_latch(e, n)) {
        // the results of the forwards issued since the last synchronisation are invalid.  One forward: re-issue it (its inputs are
        // caller-owned and untouched) on the unfused path; a burst of several cannot be re-issued from here
        const int burst = e->fwd_since_sync;
        std::function<int()> replay = std::move(e->replay_last);
        // work enqueued BEHIND the forward (finalize, a prox step, a copy) has consumed its invalid output: re-issuing the forward alone would leave
        // that work wrong (or overwrite what it wrote in place) -- only a forward that is still the last thing on the stream is replayed
        const bool trailing = e->enqueue_serial() != e->replay_serial;
        e->fwd_since_sync = 0; e->replay_last = nullptr;
        if (burst != 1 || !replay || trailing)
            return fail(e, Status{DPIR_ERR_HIP, "conv7 fused emission timed out " + (burst == 0 ? std::string("inside a loop call (dpir_run_dps_loop)") :
                                                burst == 1 ? std::string("in a forward that other work was already queued behind (or whose buffers were freed)") :
                                                "during a burst of " + std::to_string(burst) + " un-synchronised forwards") + ": the results since the last "
                                                "synchronisation are invalid.  The hop is now off for this engine; re-issue the call(s) (not a sticky error)"});
        if (int rc = replay()) return rc;
        e->fwd_since_sync = 0; e->replay_last = nullptr;
        if (int rc = read_range(e, &n)) return rc;
    }
    e->fwd_since_sync = 0; e->replay_last = nullptr;
    if (n == 0) return DPIR_OK;
    return fail(e, Status{DPIR_ERR_RANGE, std::string(e->precision == 2 ? "f16x1" : "f16x3") + " precision mode: " + std::to_string(n) +
                                          " activation lane(s) exceeded the f16 operand range (|v| > 65000 or NaN) and were clamped since the "
                                          "last forward / loop started -- results are invalid; rerun with precision f32 (engine_precision: f32)"});
}
static int check_range(dpir_engine* e) { return dpir_check_range(e); }
// a new forward / loop starts a new accounting period (stream-ordered)
// Only the range count (bits 0..39) restarts: the fused-hop time-out count above it stays until dpir_check_range has seen it, so a time-out in an
// EARLIER forward of an un-synchronised burst is not wiped by the next forward's clear.
__global__ void range_clear_kernel(unsigned long long* ctr) { *ctr &= ~((1ull << 40) - 1ull); }
static void range_clear(dpir_engine* e) {
    if (e->range_ctr && e->precision != 0) hipLaunchKernelGGL(range_clear_kernel, dim3(1), dim3(1), 0, e->stream, e->range_ctr);
}
Status dpir_engine::resizer(int in_len, int sf, ResizerTab* out) {
    auto key = std::make_pair(in_len, sf);
    auto it = resizers.find(key);
    if (it != resizers.end()) { *out = it->second; return Status{}; }
    if (sf < 1 || in_len % sf) return invalid("Resizer: length not divisible by sf");
    ResizerTab t; t.in_len = in_len; t.out_len = in_len / sf;
    std::vector<float> w; std::vector<int> idx;
    resizer_band(in_len, t.out_len, 1.0 / sf, w, idx, t.taps);
    void *dw = nullptr, *di = nullptr;
    DPIR_HIP(hipMalloc(&dw, w.size() * sizeof(float)));
    DPIR_HIP(hipMalloc(&di, idx.size() * sizeof(int)));
    DPIR_HIP(hipMemcpy(dw, w.data(), w.size() * sizeof(float), hipMemcpyHostToDevice));
    DPIR_HIP(hipMemcpy(di, idx.data(), idx.size() * sizeof(int), hipMemcpyHostToDevice));
    t.w = reinterpret_cast<float*>(dw); t.idx = reinterpret_cast<int*>(di);
    resizers[key] = t;
    *out = t;
    return Status{};
}

Status dpir::capture_graph(dpir_engine* e, const std::function<Status()>& record, hipGraphExec_t* out) {
    bool prof_on = e->prof.on, taps_on = e->collect_taps;
    e->prof.on = false; e->collect_taps = false; e->ws.frozen = true;
    hipGraph_t graph = nullptr;
    Status cs;
    hipError_t herr = hipStreamBeginCapture(e->stream, hipStreamCaptureModeThreadLocal);
    if (herr != hipSuccess) cs = Status{DPIR_ERR_HIP, std::string("hipStreamBeginCapture: ") + hipGetErrorString(herr)};
    else {
        cs = record();
        herr = hipStreamEndCapture(e->stream, &graph);
        if (cs.ok() && herr != hipSuccess) cs = Status{DPIR_ERR_HIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(herr)};
    }
    e->ws.frozen = false; e->prof.on = prof_on; e->collect_taps = taps_on;
    if (!cs.ok()) { if (graph) (void)hipGraphDestroy(graph); return cs; }
    herr = hipGraphInstantiate(out, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (herr != hipSuccess) return Status{DPIR_ERR_HIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(herr)};
    return Status{};
}

// The one shape check of the stepwise entries, made ahead of any arithmetic, allocation or launch: B, H, W >= 1 (a negative count would
// become a huge size_t element count handed to a kernel), one image's pixel count within the int the kernels decode it with, and, where
// the entry has a scale factor, sf >= 1 dividing H and W (H / sf is formed on the host).  sf = 1 for the entries without one.
static Status check_shape(const char* entry, int B, int H, int W, int sf = 1) {
    if (B < 1 || H < 1 || W < 1)
        return invalid(std::string(entry) + ": B, H and W must be >= 1 (got B " + std::to_string(B) + ", H " + std::to_string(H) + ", W " + std::to_string(W) + ")");
    if ((long long)H * W > 0x7fffffffLL / 4) return invalid(std::string(entry) + ": H * W is out of range");
    if (sf < 1 || H % sf || W % sf)
        return invalid(std::string(entry) + ": sf must be >= 1 and divide H and W (got sf " + std::to_string(sf) + ", H " + std::to_string(H) + ", W " + std::to_string(W) + ")");
    return Status{};
}

// ---- progressive strip (dpir_set_progress): shared by the four whole-loop entries
// The arming lasts for ONE public loop call: cleared when that call returns, whatever it returns (a re-run by run_with_hop_guard happens inside it).
struct ProgressOneShot {
    dpir_engine* e;
    ~ProgressOneShot() { if (e) e->progress = dpir_engine::Progress{}; }
};
// before anything is launched: the armed table must describe this call
static Status progress_check(dpir_engine* e, const char* entry, int n_entries, const dpir_loop_desc& d) {
    const dpir_engine::Progress& pg = e->progress;
    if (!pg.armed) return Status{};
    if ((int)pg.panel_of.size() != n_entries)
        return invalid(std::string(entry) + ": dpir_set_progress armed " + std::to_string(pg.panel_of.size()) + " entries for a loop of " + std::to_string(n_entries));
    if ((pg.masked_f32 || pg.masked_u8) && (!d.mask_dev || !d.y_dev || d.sf != 1))
        return invalid(std::string(entry) + ": a masked progress strip needs the mask and a full-size y (inpainting)");
    if ((long long)pg.n_panels * d.W > 0x7fffffffLL) return invalid(std::string(entry) + ": n_panels * W is out of range");
    return Status{};
}
// the panel of step / row idx, if it has one, from x as it stands on the stream now
static Status progress_emit(dpir_engine* e, int idx, const float* x, const dpir_loop_desc& d) {
    const dpir_engine::Progress& pg = e->progress;
    if (!pg.armed || idx < 0 || pg.panel_of[idx] < 0) return Status{};
    ProfScope ps(&e->prof, PC_ELEM);
    const bool masked = pg.masked_f32 || pg.masked_u8;
    ProgressArgs a{x, masked ? d.y_dev : nullptr, masked ? d.mask_dev : nullptr, pg.strip_f32, pg.strip_u8, pg.masked_f32, pg.masked_u8, pg.minmax,
                   d.B, d.H, d.W, pg.panel_of[idx], pg.n_panels, e->cus};
    return launch_progress_snapshot(e->stream, a);
}

extern "C" {

int dpir_version(void) { return DPIR_ABI_VERSION; }

int dpir_device_count(int* n_out) {
    if (!n_out) return DPIR_ERR_INVALID;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess) { (void)hipGetLastError(); count = 0; }
    *n_out = count;
    return DPIR_OK;
}

int dpir_device_info(dpir_engine* e, char* buf, size_t cap) {
    if (!e || !buf || cap == 0) return DPIR_ERR_INVALID;
    hipDeviceProp_t p;
    if (hipGetDeviceProperties(&p, e->device) != hipSuccess) return fail(e, Status{DPIR_ERR_HIP, "hipGetDeviceProperties failed"});
    char bus[32] = "?";
    (void)hipDeviceGetPCIBusId(bus, sizeof(bus), e->device);
    snprintf(buf, cap, "%s | %s | pci %s | %d CUs | ordinal %d", p.gcnArchName, p.name, bus, p.multiProcessorCount, e->device);
    return DPIR_OK;
}

int dpir_create(int device, dpir_engine** out) {
    if (!out) return DPIR_ERR_INVALID;
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count) return DPIR_ERR_HIP;
    if (hipSetDevice(device) != hipSuccess) return DPIR_ERR_HIP;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return DPIR_ERR_HIP;
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return DPIR_ERR_UNSUPPORTED;   // kernels are built for gfx950 only
    dpir_engine* e = new (std::nothrow) dpir_engine();
    if (!e) return DPIR_ERR_NOMEM;
    e->device = device;
    if (hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking) != hipSuccess) { delete e; return DPIR_ERR_HIP; }
    e->prof.stream = e->stream;
    if (hipMalloc((void**)&e->range_ctr, sizeof(unsigned long long)) != hipSuccess ||
        hipMemset(e->range_ctr, 0, sizeof(unsigned long long)) != hipSuccess) { (void)hipStreamDestroy(e->stream); delete e; return DPIR_ERR_NOMEM; }
    e->cus = prop.multiProcessorCount;
    if (const char* ev = getenv("DPIR_PROX_MODE")) { const int m = atoi(ev); if (m >= 0 && m <= 3) e->prox_mode = m; }
    *out = e;
    return DPIR_OK;
}

void dpir_destroy(dpir_engine* e) {
    if (!e) return;
    (void)hipSetDevice(e->device);
    (void)hipStreamSynchronize(e->stream);
    unet_free(e);
    e->ws.release();
    e->prox_cache.release();
    for (auto& kv : e->resizers) { (void)hipFree(kv.second.w); (void)hipFree(kv.second.idx); }
    for (void* p : e->user_allocs) (void)hipFree(p);
    e->invalidate_graphs();
    prox_release(&e->loop_prox);
    (void)dpir_comm_destroy(e);
    if (e->range_ctr) (void)hipFree(e->range_ctr);
    if (e->progress_premix) (void)hipFree(e->progress_premix);
    lpips_free(e);
    fid_free(e);
    if (e->metrics8_buf) (void)hipFree(e->metrics8_buf);
    (void)hipStreamDestroy(e->stream);
    delete e;
}

const char* dpir_last_error(const dpir_engine* e) { return e ? e->last_error.c_str() : "null engine"; }

int dpir_sync(dpir_engine* e) {
    if (!e) return DPIR_ERR_INVALID;
    API_HIP(e, hipStreamSynchronize(e->stream));
    return check_range(e);
}
void* dpir_stream(dpir_engine* e) { return e ? (void*)e->stream : nullptr; }

int dpir_malloc(dpir_engine* e, size_t bytes, void** dev_out) {
    if (!e || !dev_out) return DPIR_ERR_INVALID;
    (void)hipSetDevice(e->device);
    void* p = nullptr;
    if (hipMalloc(&p, bytes ? bytes : 1) != hipSuccess) return fail(e, Status{DPIR_ERR_NOMEM, "dpir_malloc: hipMalloc failed"});
    e->user_allocs.push_back(p);
    *dev_out = p;
    return DPIR_OK;
}
int dpir_free(dpir_engine* e, void* dev) {
    if (!e) return DPIR_ERR_INVALID;
    for (size_t i = 0; i < e->user_allocs.size(); ++i)
        if (e->user_allocs[i] == dev) {
            (void)hipStreamSynchronize(e->stream);
            ++e->copy_serial;                      // a pending forward replay may hold this pointer: it is no longer valid (dpir_check_range)
            (void)hipFree(dev);
            e->user_allocs.erase(e->user_allocs.begin() + i);
            return DPIR_OK;
        }
    return fail(e, invalid("dpir_free: pointer was not allocated by dpir_malloc"));
}
int dpir_h2d(dpir_engine* e, void* d, const void* h, size_t bytes) {
    if (!e) return DPIR_ERR_INVALID;
    ++e->copy_serial;
    API_HIP(e, hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, e->stream));
    API_HIP(e, hipStreamSynchronize(e->stream));   // the host buffer may be pageable / short-lived
    return DPIR_OK;
}
int dpir_d2h(dpir_engine* e, void* h, const void* d, size_t bytes) {
    if (!e) return DPIR_ERR_INVALID;
    // the guard word FIRST: a fused-hop time-out re-issues the invalidated forward (dpir_check_range), and the copy must see its result
    if (int rc = check_range(e)) return rc;
    API_HIP(e, hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, e->stream));
    API_HIP(e, hipStreamSynchronize(e->stream));
    return DPIR_OK;
}
int dpir_d2d(dpir_engine* e, void* dd, const void* ds, size_t bytes) {
    if (!e) return DPIR_ERR_INVALID;
    ++e->copy_serial;
    API_HIP(e, hipMemcpyAsync(dd, ds, bytes, hipMemcpyDeviceToDevice, e->stream));
    return DPIR_OK;
}

// ------------------------------------------------------------------------------------------ UNet
int dpir_load_unet(dpir_engine* e, const dpir_unet_desc* desc, const dpir_tensor* weights, int n_weights) {
    if (!e || !desc || !weights || n_weights <= 0) return fail(e, invalid("dpir_load_unet: null argument"));
    (void)hipSetDevice(e->device);
    API_HIP(e, hipStreamSynchronize(e->stream));
    e->invalidate_graphs();
    Status s = unet_load(e, desc, weights, n_weights);
    if (!s.ok()) { unet_free(e); return fail(e, s); }
    return DPIR_OK;
}

static Status upload_ints(dpir_engine* e, const char* name, const int64_t* host, int B, int** dev) {
    if (!host) { *dev = nullptr; return Status{}; }
    DPIR_TRY(e->ws.getT(name, (size_t)B, dev));
    std::vector<int> tmp(B);
    for (int i = 0; i < B; ++i) tmp[i] = (int)host[i];
    DPIR_HIP(hipMemcpyAsync(*dev, tmp.data(), B * sizeof(int), hipMemcpyHostToDevice, e->stream));
    DPIR_HIP(hipStreamSynchronize(e->stream));
    return Status{};
}
static Status labels_match(const dpir_engine* e, const int64_t* labels_host) {
    return (e->net.desc.num_classes > 0) != (labels_host != nullptr) ? invalid("labels iff class-conditional model") : Status{};
}

// One timestep for the whole batch (what model_fn passes): written on the device by a 1-workgroup kernel -- no host buffer, no copy and, unlike
// upload_ints, no hipStreamSynchronize, so back-to-back eager forwards are queued while the previous one still runs.
__global__ void fill_const_kernel(int* p, int v, int n) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}
static Status fill_ints(dpir_engine* e, const char* name, int value, int B, int** dev) {
    DPIR_TRY(e->ws.getT(name, (size_t)B, dev));
    hipLaunchKernelGGL(fill_const_kernel, dim3((B + 255) / 256), dim3(256), 0, e->stream, *dev, value, B);
    DPIR_HIP(hipGetLastError());
    return Status{};
}

int dpir_set_precision(dpir_engine* e, int mode) {
    if (!e) return DPIR_ERR_INVALID;
    if (mode < 0 || mode > 2) return fail(e, invalid("dpir_set_precision: mode must be 0 (fp32 MFMA), 1 (operand-split f16x3 MFMA) or 2 (f16x1: f16 operands, fp32 accumulate)"));
    if (e->net.loaded && mode != e->precision) return fail(e, Status{DPIR_ERR_STATE, "dpir_set_precision must be called before dpir_load_unet"});
    e->precision = mode;
    return DPIR_OK;
}

int dpir_unet_forward(dpir_engine* e, const float* x, const int64_t* t_host, const int64_t* y_host, float* out, int B, int H, int W) {
    if (!e || !x || !t_host || !out) return fail(e, invalid("dpir_unet_forward: null argument"));
    (void)hipSetDevice(e->device);
    int *t_dev = nullptr, *y_dev = nullptr;
    range_clear(e);
    bool uni = true;
    for (int i = 1; i < B; ++i) uni = uni && t_host[i] == t_host[0];
    if (uni && !y_host) API_TRY(e, fill_ints(e, "api#t", (int)t_host[0], B, &t_dev));
    else API_TRY(e, upload_ints(e, "api#t", t_host, B, &t_dev));
    API_TRY(e, upload_ints(e, "api#y", y_host, B, &y_dev));
    if (y_host && e->net.loaded)
        for (int i = 0; i < B; ++i)
            if (y_host[i] < 0 || y_host[i] >= e->net.desc.num_classes) return fail(e, invalid("class label out of range"));
    API_TRY(e, unet_forward(e, x, t_dev, y_dev, out, B, H, W, nullptr, nullptr, uni));
    if (!e->fuse_h1_off && !e->grad_enabled && e->precision != 0) {
        std::vector<int64_t> tv(t_host, t_host + B), yv;
        if (y_host) yv.assign(y_host, y_host + B);
        if (x != out) e->arm_replay([=]() { return dpir_unet_forward(e, x, tv.data(), yv.empty() ? nullptr : yv.data(), out, B, H, W); });
        else { ++e->fwd_since_sync; e->replay_last = nullptr; }         // in place: the input is gone, nothing to re-issue from
    }
    return DPIR_OK;
}

int dpir_model_fn_xstart(dpir_engine* e, const float* x, int t, float c1, float c2, const int64_t* y_host, float* x0, int B, int H, int W) {
    if (!e || !x || !x0) return fail(e, invalid("dpir_model_fn_xstart: null argument"));
    (void)hipSetDevice(e->device);
    if (!e->net.loaded) return fail(e, Status{DPIR_ERR_STATE, "dpir_load_unet has not been called"});
    int *t_dev = nullptr, *y_dev = nullptr;
    range_clear(e);
    API_TRY(e, fill_ints(e, "api#t", t, B, &t_dev));
    API_TRY(e, upload_ints(e, "api#y", y_host, B, &y_dev));
    float* out6 = nullptr;
    API_TRY(e, e->ws.getT("api#out6", (size_t)B * e->net.desc.out_channels * H * W, &out6));
    API_TRY(e, unet_forward(e, x, t_dev, y_dev, out6, B, H, W, nullptr, nullptr, true));
    ProfScope ps(&e->prof, PC_ELEM);
    API_TRY(e, launch_xstart(e->stream, x, out6, e->net.desc.out_channels, c1, c2, x0, B, H * W));
    if (!e->fuse_h1_off && !e->grad_enabled && e->precision != 0) {
        std::vector<int64_t> yv;
        if (y_host) yv.assign(y_host, y_host + B);
        if (x != x0) e->arm_replay([=]() { return dpir_model_fn_xstart(e, x, t, c1, c2, yv.empty() ? nullptr : yv.data(), x0, B, H, W); });
        else { ++e->fwd_since_sync; e->replay_last = nullptr; }
    }
    return DPIR_OK;
}

int dpir_unet_read_tap(dpir_engine* e, const char* layer, float* host_dst, size_t cap, size_t* numel_out) {
    if (!e || !layer) return fail(e, invalid("dpir_unet_read_tap: null argument"));
    auto it = e->taps.find(layer);
    if (it == e->taps.end()) return fail(e, invalid(std::string("no such tap: ") + layer));
    if (numel_out) *numel_out = it->second.numel;
    if (!host_dst) return DPIR_OK;
    if (cap < it->second.numel) return fail(e, invalid("dpir_unet_read_tap: destination too small"));
    return dpir_d2h(e, host_dst, it->second.p, it->second.numel * sizeof(float));
}

double dpir_unet_flops(dpir_engine* e, int H, int W) { return e ? unet_flops(e->net, H, W) : 0.0; }
double dpir_unet_flops_class(dpir_engine* e, int H, int W, int cls) { return e ? unet_flops(e->net, H, W, cls) : 0.0; }

// ------------------------------------------------------------------------------------------ gradient mode (8f-4)
int dpir_enable_grad(dpir_engine* e, int on) {
    if (!e) return DPIR_ERR_INVALID;
    if (e->net.loaded && (on != 0) != e->grad_enabled) return fail(e, Status{DPIR_ERR_STATE, "dpir_enable_grad must be called before dpir_load_unet"});
    e->grad_enabled = on != 0;
    return DPIR_OK;
}

int dpir_unet_vjp(dpir_engine* e, const float* x, const int64_t* t_host, const int64_t* y_host, const float* gout, float* out, float* dx,
                  int B, int H, int W) {
    if (!e || !x || !t_host || !gout || !dx) return fail(e, invalid("dpir_unet_vjp: null argument"));
    (void)hipSetDevice(e->device);
    if (!e->grad_enabled) return fail(e, Status{DPIR_ERR_STATE, "dpir_unet_vjp: gradient mode is off (dpir_enable_grad before dpir_load_unet)"});
    int *t_dev = nullptr, *y_dev = nullptr;
    range_clear(e);
    API_TRY(e, upload_ints(e, "api#t", t_host, B, &t_dev));
    API_TRY(e, upload_ints(e, "api#y", y_host, B, &y_dev));
    float* o6 = out;
    if (!o6) API_TRY(e, e->ws.getT("api#out6", (size_t)B * e->net.desc.out_channels * H * W, &o6));
    API_TRY(e, unet_forward(e, x, t_dev, y_dev, o6, B, H, W));
    API_TRY(e, unet_backward(e, gout, dx));
    return DPIR_OK;
}

// ------------------------------------------------------------------------------------------ FFT prox (prox.hip)
int dpir_prox_fft_precalc(dpir_engine* e, const float* y, const float* k, int kh, int kw, int sf, int B, int H, int W, dpir_prox** out) {
    if (!e || !y || !k || !out) return fail(e, invalid("dpir_prox_fft_precalc: null argument"));
    (void)hipSetDevice(e->device);
    *out = nullptr;
    dpir_prox* p = new (std::nothrow) dpir_prox();
    if (!p) return fail(e, Status{DPIR_ERR_NOMEM, "out of host memory"});
    Status s = prox_create(e, y, k, kh, kw, sf, B, H, W, &p->st);
    if (!s.ok()) { delete p; return fail(e, s); }
    *out = p;
    return DPIR_OK;
}
void dpir_prox_free(dpir_engine* e, dpir_prox* p) {
    if (!p) return;
    if (e) (void)hipStreamSynchronize(e->stream);
    prox_release(&p->st);
    delete p;
}

int dpir_prox_read(dpir_engine* e, const dpir_prox* p, int which, void* host_dst, size_t cap_bytes) {
    if (!e || !p || !host_dst) return fail(e, invalid("dpir_prox_read: null argument"));
    API_TRY(e, prox_read(e, p->st, which, host_dst, cap_bytes));
    return DPIR_OK;
}

int dpir_set_prox_launch(dpir_engine* e, int mode) {
    if (!e || mode < 0 || mode > 3) return fail(e, invalid("dpir_set_prox_launch: mode must be 0, 1, 2 or 3"));
    (void)hipSetDevice(e->device);
    if (mode != e->prox_mode) { (void)hipStreamSynchronize(e->stream); e->invalidate_graphs(); }
    e->prox_mode = mode;
    return DPIR_OK;
}
int dpir_data_solution(dpir_engine* e, const dpir_prox* p, const float* x, float alpha, float* out) {
    if (!e || !p || !x || !out) return fail(e, invalid("dpir_data_solution: null argument"));
    (void)hipSetDevice(e->device);
    API_TRY(e, prox_data_solution(e, p->st, x, 1.f, 0.f, alpha, out, 1.f, 0.f, nullptr, 0.f));
    return DPIR_OK;
}
int dpir_prox_fft_apply(dpir_engine* e, const dpir_prox* p, float* x0, float tau, float guidance) {
    if (!e || !p || !x0) return fail(e, invalid("dpir_prox_fft_apply: null argument"));
    (void)hipSetDevice(e->device);
    API_TRY(e, prox_data_solution(e, p->st, x0, 0.5f, 0.5f, tau, x0, 2.f, -1.f, x0, guidance));
    return DPIR_OK;
}
int dpir_prox_fft_apply_timed(dpir_engine* e, const dpir_prox* p, float* x0, float tau, float guidance, int n, int use_graph, float* us_per_apply) {
    if (!e || !p || !x0 || !us_per_apply || n < 1) return fail(e, invalid("dpir_prox_fft_apply_timed: bad argument"));
    (void)hipSetDevice(e->device);
    API_TRY(e, prox_apply_timed(e, p->st, x0, tau, guidance, n, use_graph != 0, us_per_apply));
    return DPIR_OK;
}

int dpir_prox_mask(dpir_engine* e, float* x0, const float* y, const uint8_t* mask, float tau, float guidance, int B, int H, int W) {
    if (!e || !x0 || !y || !mask) return fail(e, invalid("dpir_prox_mask: null argument"));
    API_TRY(e, check_shape("dpir_prox_mask", B, H, W));
    (void)hipSetDevice(e->device);
    ProfScope ps(&e->prof, PC_ELEM);
    API_TRY(e, launch_prox_mask(e->stream, x0, y, mask, tau, guidance, (size_t)B * 3 * H * W));
    return DPIR_OK;
}

static Status resize_down_impl(dpir_engine* e, const float* x, float pa, float pb, float* out, int sf, int B, int H, int W) {
    ResizerTab th, tw;
    DPIR_TRY(e->resizer(H, sf, &th));
    DPIR_TRY(e->resizer(W, sf, &tw));
    float* mid = nullptr;
    DPIR_TRY(e->ws.getT("resize#mid", (size_t)B * 3 * (H / sf) * W, &mid));
    ProfScope ps(&e->prof, PC_ELEM);
    // dim 2 (H) first, then dim 3 (W): utils_resizer.py:29-30 (stable argsort of equal scale factors)
    DPIR_TRY(launch_band_resample(e->stream, x, th.w, th.idx, th.taps, B * 3, H, H / sf, W, pa, pb, mid));
    DPIR_TRY(launch_band_resample(e->stream, mid, tw.w, tw.idx, tw.taps, B * 3 * (H / sf), W, W / sf, 1, 1.f, 0.f, out));
    return Status{};
}

int dpir_resize_down(dpir_engine* e, const float* x, float* out, int sf, int B, int H, int W) {
    if (!e || !x || !out) return fail(e, invalid("dpir_resize_down: null argument"));
    API_TRY(e, check_shape("dpir_resize_down", B, H, W, sf));
    (void)hipSetDevice(e->device);
    API_TRY(e, resize_down_impl(e, x, 1.f, 0.f, out, sf, B, H, W));
    return DPIR_OK;
}

static Status prox_ibp_impl(dpir_engine* e, float* x0, const float* y, float rho, float gamma, int in_iter, int sf, int B, int H, int W,
                            const StepDev* sp = nullptr, const LoopDev* lp = nullptr, bool per_image = false) {
    float* d = nullptr;
    DPIR_TRY(e->ws.getT("ibp#down", (size_t)B * 3 * (H / sf) * (W / sf), &d));
    for (int it = 0; it < in_iter; ++it) {
        DPIR_TRY(resize_down_impl(e, x0, 0.5f, 0.5f, d, sf, B, H, W));      // down(x0/2+.5)
        ProfScope ps(&e->prof, PC_ELEM);
        DPIR_TRY(launch_ibp_update(e->stream, x0, y, d, gamma, rho, sf, B * 3, H, W, sp, lp, per_image));
    }
    return Status{};
}
int dpir_prox_ibp(dpir_engine* e, float* x0, const float* y, float rho, float gamma, int in_iter, int sf, int B, int H, int W) {
    if (!e || !x0 || !y) return fail(e, invalid("dpir_prox_ibp: null argument"));
    API_TRY(e, check_shape("dpir_prox_ibp", B, H, W, sf));
    (void)hipSetDevice(e->device);
    API_TRY(e, prox_ibp_impl(e, x0, y, rho, gamma, in_iter, sf, B, H, W));
    return DPIR_OK;
}

int dpir_bicubic_up(dpir_engine* e, const float* y, float* out, int sf, int B, int h, int w) {
    if (!e || !y || !out) return fail(e, invalid("dpir_bicubic_up: null argument"));
    API_TRY(e, check_shape("dpir_bicubic_up", B, h, w));
    // h sf and w sf are bounded one by one first: their product then fits a long long
    if (sf < 1 || (long long)h * sf > 0x7fffffffLL || (long long)w * sf > 0x7fffffffLL || ((long long)h * sf) * ((long long)w * sf) > 0x7fffffffLL / 4)
        return fail(e, invalid("dpir_bicubic_up: sf must be >= 1 and (h sf) * (w sf) in range"));
    (void)hipSetDevice(e->device);
    ProfScope ps(&e->prof, PC_ELEM);
    API_TRY(e, launch_bicubic_up(e->stream, y, out, B * 3, h, w, sf));
    return DPIR_OK;
}

// ------------------------------------------------------------------------------------------ loop arithmetic
// First-order data step of the DiffPIR loop (sub_1_analytic: false, main_ddpir.py:420-430; task sr):
//   x0 <- x0 - d|| (2y - 1) - Resizer(x0) || / dx0 * ||.|| / rho       -- the gradient needs no network backward
static Status prox_first_order_impl(dpir_engine* e, float* x0, const float* y, float rho, int sf, int B, int H, int W,
                                    const StepDev* sp = nullptr, const LoopDev* lp = nullptr) {
    const int h = H / sf, w = W / sf;
    const size_t total = (size_t)B * 3 * H * W, small = (size_t)B * 3 * h * w;
    float *down = nullptr, *diff = nullptr, *gmid = nullptr, *gup = nullptr, *normv = nullptr; double* part = nullptr;
    DPIR_TRY(e->ws.getT("fo#down", small, &down));
    DPIR_TRY(e->ws.getT("fo#diff", small, &diff));
    DPIR_TRY(e->ws.getT("fo#gmid", (size_t)B * 3 * h * W, &gmid));
    DPIR_TRY(e->ws.getT("fo#gup", total, &gup));
    DPIR_TRY(e->ws.getT("fo#part", (size_t)256, &part));
    DPIR_TRY(e->ws.getT("fo#norm", (size_t)4, &normv));
    ResizerTab th, tw;
    DPIR_TRY(e->resizer(H, sf, &th));
    DPIR_TRY(e->resizer(W, sf, &tw));
    DPIR_TRY(resize_down_impl(e, x0, 1.f, 0.f, down, sf, B, H, W));
    ProfScope ps(&e->prof, PC_ELEM);
    hipStream_t s = e->stream;
    DPIR_TRY(launch_diff_norm(s, y, 2.f, -1.f, down, diff, small, part, 256, normv, 1.f, 0.f, nullptr, lp));
    DPIR_TRY(launch_band_resample_T(s, diff, tw.w, tw.idx, tw.taps, B * 3 * h, W, w, 1, 1.f, gmid));
    DPIR_TRY(launch_band_resample_T(s, gmid, th.w, th.idx, th.taps, B * 3, H, h, W, 1.f, gup));
    DPIR_TRY(launch_grad_step(s, x0, gup, normv, 1.f, rho, 1.f, x0, total, sp));
    return Status{};
}

static RenoiseCoef coef_of(const dpir_step& s) { return RenoiseCoef{s.sa_t, s.s1m_t, s.sa_p, s.k1, s.q, s.es, s.k2}; }

int dpir_renoise(dpir_engine* e, float* x, const float* x0, const dpir_step* s, const float* n1, const float* n2, int B, int H, int W) {
    if (!e || !x || !x0 || !s || !n2) return fail(e, invalid("dpir_renoise: null argument"));
    if (s->es != 0.f && !n1) return fail(e, invalid("dpir_renoise: eta_sigma != 0 needs n1"));
    API_TRY(e, check_shape("dpir_renoise", B, H, W));
    (void)hipSetDevice(e->device);
    ProfScope ps(&e->prof, PC_ELEM);
    API_TRY(e, launch_renoise(e->stream, x, x0, coef_of(*s), s->es != 0.f ? n1 : nullptr, n2, (size_t)B * 3 * H * W));
    return DPIR_OK;
}
int dpir_repaint_mix(dpir_engine* e, float* x, const float* y, const uint8_t* mask, const dpir_step* s, const float* n, int B, int H, int W) {
    if (!e || !x || !y || !mask || !s || !n) return fail(e, invalid("dpir_repaint_mix: null argument"));
    API_TRY(e, check_shape("dpir_repaint_mix", B, H, W));
    (void)hipSetDevice(e->device);
    ProfScope ps(&e->prof, PC_ELEM);
    API_TRY(e, launch_repaint_mix(e->stream, x, y, mask, n, s->sa_t, s->s1m_t, (size_t)B * 3 * H * W));
    return DPIR_OK;
}
int dpir_finalize(dpir_engine* e, const float* x, float* of, uint8_t* ou, int B, int H, int W) {
    if (!e || !x) return fail(e, invalid("dpir_finalize: null argument"));
    API_TRY(e, check_shape("dpir_finalize", B, H, W));
    (void)hipSetDevice(e->device);
    ProfScope ps(&e->prof, PC_ELEM);
    API_TRY(e, launch_finalize(e->stream, x, of, ou, B, H * W));
    return DPIR_OK;
}
int dpir_progress_snapshot(dpir_engine* e, const float* x, const float* y, const uint8_t* mask, int panel, int n_panels, float* strip_f32,
                           uint8_t* strip_u8, float* masked_f32, uint8_t* masked_u8, float* minmax, int B, int H, int W) {
    if (!e || !x) return fail(e, invalid("dpir_progress_snapshot: null argument"));
    API_TRY(e, check_shape("dpir_progress_snapshot", B, H, W));
    if (n_panels < 1 || panel < 0 || panel >= n_panels)
        return fail(e, invalid("dpir_progress_snapshot: panel must be in [0, n_panels) (got panel " + std::to_string(panel) + " of " + std::to_string(n_panels) + ")"));
    if ((long long)n_panels * W > 0x7fffffffLL) return fail(e, invalid("dpir_progress_snapshot: n_panels * W is out of range"));
    const bool masked = masked_f32 || masked_u8;
    if (masked && (!y || !mask)) return fail(e, invalid("dpir_progress_snapshot: a masked output needs y and mask"));
    if (reinterpret_cast<uintptr_t>(minmax) & 3u) return fail(e, invalid("dpir_progress_snapshot: minmax must be 4-byte aligned"));
    (void)hipSetDevice(e->device);
    ProfScope ps(&e->prof, PC_ELEM);
    ProgressArgs a{x, masked ? y : nullptr, masked ? mask : nullptr, strip_f32, strip_u8, masked_f32, masked_u8, minmax, B, H, W, panel, n_panels, e->cus};
    API_TRY(e, launch_progress_snapshot(e->stream, a));
    return DPIR_OK;
}
int dpir_set_progress(dpir_engine* e, const dpir_progress_desc* desc) {
    if (!e) return DPIR_ERR_INVALID;
    e->progress = dpir_engine::Progress{};
    if (!desc) return DPIR_OK;
    if (!desc->panel_of_step_host || desc->n_entries < 1 || desc->n_panels < 1) return fail(e, invalid("dpir_set_progress: the panel table, n_entries and n_panels are required"));
    if (reinterpret_cast<uintptr_t>(desc->minmax_dev) & 3u) return fail(e, invalid("dpir_set_progress: minmax_dev must be 4-byte aligned"));
    for (int i = 0; i < desc->n_entries; ++i)
        if (desc->panel_of_step_host[i] < -1 || desc->panel_of_step_host[i] >= desc->n_panels)
            return fail(e, invalid("dpir_set_progress: entry " + std::to_string(i) + " is outside [-1, n_panels)"));
    dpir_engine::Progress& pg = e->progress;
    pg.panel_of.assign(desc->panel_of_step_host, desc->panel_of_step_host + desc->n_entries);
    pg.n_panels = desc->n_panels;
    pg.strip_f32 = desc->strip_f32; pg.strip_u8 = desc->strip_u8; pg.masked_f32 = desc->masked_f32; pg.masked_u8 = desc->masked_u8; pg.minmax = desc->minmax_dev;
    pg.armed = true;
    return DPIR_OK;
}
int dpir_randn(dpir_engine* e, float* out, uint64_t seed, uint64_t stream_id, int64_t image_offset, int B, int C, int H, int W) {
    if (!e || !out) return fail(e, invalid("dpir_randn: null argument"));
    API_TRY(e, check_shape("dpir_randn", B, H, W));
    if (C < 1 || (long long)C * H * W > 0x7fffffffLL) return fail(e, invalid("dpir_randn: C must be >= 1 and C * H * W in range"));
    (void)hipSetDevice(e->device);
    ProfScope ps(&e->prof, PC_ELEM);
    API_TRY(e, launch_randn(e->stream, out, seed, stream_id, image_offset, B, (size_t)C * H * W));
    return DPIR_OK;
}

int dpir_randn_indexed(dpir_engine* e, float* out, uint64_t seed, uint64_t stream_id, const int64_t* image_index, int B, int C, int H, int W) {
    if (!e || !out || !image_index) return fail(e, invalid("dpir_randn_indexed: null argument"));
    API_TRY(e, check_shape("dpir_randn_indexed", B, H, W));
    if (C < 1 || (long long)C * H * W > 0x7fffffffLL) return fail(e, invalid("dpir_randn_indexed: C must be >= 1 and C * H * W in range"));
    (void)hipSetDevice(e->device);
    long long* idx = nullptr;
    API_TRY(e, e->ws.getT("randn#idx", (size_t)B, &idx));
    static_assert(sizeof(long long) == sizeof(int64_t), "the image numbers are copied as they are");
    API_HIP(e, hipMemcpyAsync(idx, image_index, sizeof(int64_t) * B, hipMemcpyHostToDevice, e->stream));
    API_HIP(e, hipStreamSynchronize(e->stream));        // the host array is the caller's
    ProfScope ps(&e->prof, PC_ELEM);
    API_TRY(e, launch_randn(e->stream, out, seed, stream_id, 0, B, (size_t)C * H * W, nullptr, nullptr, idx));
    return DPIR_OK;
}

int dpir_ewise(dpir_engine* e, int op, const float* x_dev, const float* y_dev, size_t y_numel, float scalar, float* out_dev, size_t numel) {
    if (!e || !x_dev || !out_dev) return fail(e, invalid("dpir_ewise: null argument"));
    (void)hipSetDevice(e->device);
    ProfScope ps(&e->prof, PC_ELEM);
    API_TRY(e, launch_ewise(e->stream, op, x_dev, y_dev, y_numel, scalar, out_dev, numel));
    return DPIR_OK;
}

// ------------------------------------------------------------------------------------------ degradation + metrics
int dpir_degrade(dpir_engine* e, const dpir_degrade_desc* d, const uint8_t* gt, const float* k, const uint8_t* mask, const float* noise, float* y) {
    if (!e || !d || !gt || !y) return fail(e, invalid("dpir_degrade: null argument"));
    (void)hipSetDevice(e->device);
    const int B = d->B, H = d->H, W = d->W, sf = d->sf < 1 ? 1 : d->sf;
    if (B <= 0 || H <= 0 || W <= 0 || H % sf || W % sf) return fail(e, invalid("dpir_degrade: bad shape"));
    hipStream_t s = e->stream;
    ProfScope ps(&e->prof, PC_ELEM);
    const int h = H / sf, w = W / sf;
    if (d->task == DPIR_TASK_DEBLUR) {
        if (!k) return fail(e, invalid("dpir_degrade: deblurring needs a PSF"));
        API_TRY(e, launch_blur_wrap_u8(s, gt, k, d->kh, d->kw, B, H, W, y));
    } else if (d->task == DPIR_TASK_INPAINT) {
        if (!mask) return fail(e, invalid("dpir_degrade: inpainting needs a mask"));      // img_H * mask / 255 is formed in the finish kernel (float64)
    } else if (d->task == DPIR_TASK_SR_BLUR || d->task == DPIR_TASK_SR_CUBIC) {
        float* full = nullptr;
        API_TRY(e, e->ws.getT("degrade#full", (size_t)B * 3 * H * W, &full));
        API_TRY(e, launch_u8_to_single(s, gt, nullptr, B, H * W, full));
        API_TRY(e, resize_down_impl(e, full, 1.f, 0.f, y, sf, B, H, W));
    } else return fail(e, invalid("dpir_degrade: unknown task"));
    const size_t total = (size_t)B * 3 * h * w;
    const float* nz = noise;
    if (!nz && d->noise_level_img != 0.f) {
        float* nb = nullptr;
        API_TRY(e, e->ws.getT("degrade#noise", total, &nb));
        // Philox stream 2^40: the loop's streams are draw + 4 * step (draw 0..3), so no (seed, image) pair can meet this one
        API_TRY(e, launch_randn(s, nb, d->seed, 1ull << 40, d->image_offset, B, (size_t)3 * h * w));
        nz = nb;
    }
    const bool inp = d->task == DPIR_TASK_INPAINT;
    API_TRY(e, launch_degrade_finish(s, y, d->noise_level_img != 0.f ? nz : nullptr, (double)d->noise_level_img * 2.0,
                                     inp ? mask : nullptr, inp ? gt : nullptr, H * W, total));
    return DPIR_OK;
}

int dpir_metrics(dpir_engine* e, const float* x0, const uint8_t* gt, int B, int H, int W, float* psnr_host, float* psnr_y_host) {
    if (!e || !x0 || !gt || !psnr_host) return fail(e, invalid("dpir_metrics: null argument"));
    API_TRY(e, check_shape("dpir_metrics", B, H, W));
    (void)hipSetDevice(e->device);
    double2* acc = nullptr;
    API_TRY(e, e->ws.getT("metrics#acc", (size_t)B, &acc));
    {
        ProfScope ps(&e->prof, PC_ELEM);
        API_TRY(e, launch_metrics(e->stream, x0, gt, B, H * W, acc));
    }
    std::vector<double2> h(B);
    int rc = dpir_d2h(e, h.data(), acc, sizeof(double2) * B);
    if (rc != DPIR_OK) return rc;
    const double cnt = 3.0 * H * W;
    for (int i = 0; i < B; ++i) {
        // utils_image.calculate_psnr_batch: inf when mse == 0, else 20*log10(max_pixel / sqrt(mse + eps)); evaluated in float64 and rounded once
        // (in float32 log10f and the final product alone cost up to 1.5e-5 dB at 85 dB)
        const double mse = h[i].x / cnt, mse_y = h[i].y / cnt;
        psnr_host[i] = mse == 0.0 ? INFINITY : (float)(20.0 * log10(2.0 / sqrt(mse + 1e-10)));
        if (psnr_y_host) psnr_y_host[i] = mse_y == 0.0 ? INFINITY : (float)(20.0 * log10(2.0 / sqrt(mse_y + 1e-10)));
    }
    return DPIR_OK;
}

int dpir_metrics_u8(dpir_engine* e, const uint8_t* est_u8, const float* est_f32, const uint8_t* gt, int B, int H, int W, int border, double* out_host) {
    if (!e || !gt || !out_host) return fail(e, invalid("dpir_metrics_u8: null argument"));
    if ((est_u8 != nullptr) == (est_f32 != nullptr)) return fail(e, invalid("dpir_metrics_u8: exactly one of est_u8_dev and est_f32_dev must be given"));
    API_TRY(e, check_shape("dpir_metrics_u8", B, H, W));
    if (border < 0) return fail(e, invalid("dpir_metrics_u8: border must be >= 0 (got " + std::to_string(border) + ")"));
    if ((long long)H - 2LL * border < kM8Taps || (long long)W - 2LL * border < kM8Taps)
        return fail(e, invalid("dpir_metrics_u8: H - 2 border and W - 2 border must be >= 11 (no valid SSIM window; got H " + std::to_string(H) + ", W " +
                               std::to_string(W) + ", border " + std::to_string(border) + ")"));
    (void)hipSetDevice(e->device);
    const size_t tiles = (size_t)metrics8_tiles(H, W, border);
    if (tiles * (size_t)B > 0x7fffffffULL) return fail(e, invalid("dpir_metrics_u8: B * tiles is out of range"));
    const size_t need = ((size_t)B * tiles + (size_t)B) * sizeof(Metrics8Sums);
    if (need > e->metrics8_bytes) {
        API_HIP(e, hipStreamSynchronize(e->stream));
        if (e->metrics8_buf) (void)hipFree(e->metrics8_buf);
        e->metrics8_buf = nullptr; e->metrics8_bytes = 0;
        if (hipMalloc(&e->metrics8_buf, need) != hipSuccess) { (void)hipGetLastError(); return fail(e, Status{DPIR_ERR_NOMEM, "dpir_metrics_u8: hipMalloc failed"}); }
        e->metrics8_bytes = need;
    }
    Metrics8Sums* partial = reinterpret_cast<Metrics8Sums*>(e->metrics8_buf);
    Metrics8Sums* sums = partial + (size_t)B * tiles;
    {
        ProfScope ps(&e->prof, PC_ELEM);
        API_TRY(e, launch_metrics8(e->stream, est_u8, est_f32, gt, B, H, W, border, partial, sums));
    }
    std::vector<Metrics8Sums> h(B);
    int rc = dpir_d2h(e, h.data(), sums, sizeof(Metrics8Sums) * B);
    if (rc != DPIR_OK) return rc;
    const double hc = H - 2 * border, wc = W - 2 * border;
    const double n_y = hc * wc, n_rgb = 3.0 * n_y, v_y = (hc - kM8Halo) * (wc - kM8Halo), v_rgb = 3.0 * v_y;
    for (int i = 0; i < B; ++i) {
        // utils_image.calculate_psnr: inf when mse == 0, else 20 * log10(255 / sqrt(mse)), float64 from the exact integer sum
        out_host[4 * i + 0] = h[i].sse == 0 ? (double)INFINITY : 20.0 * log10(255.0 / sqrt((double)h[i].sse / n_rgb));
        out_host[4 * i + 1] = h[i].sse_y == 0 ? (double)INFINITY : 20.0 * log10(255.0 / sqrt((double)h[i].sse_y / n_y));
        out_host[4 * i + 2] = h[i].ssim / v_rgb;
        out_host[4 * i + 3] = h[i].ssim_y / v_y;
    }
    return DPIR_OK;
}

int dpir_result_panels(dpir_engine* e, const dpir_result_desc* d, const float* y, const uint8_t* kv, const uint8_t* est, const uint8_t* gt,
                       uint8_t* L_u8, uint8_t* leh_u8) {
    if (!e || !d) return fail(e, invalid("dpir_result_panels: null argument"));
    API_TRY(e, check_shape("dpir_result_panels", d->B, d->H, d->W, d->sf));
    if (d->mode != 0 && d->mode != 1) return fail(e, invalid("dpir_result_panels: mode must be 0 (kernel-inset strip) or 1 (inpainting strip), got " + std::to_string(d->mode)));
    if (d->mode == 1 && d->sf != 1) return fail(e, invalid("dpir_result_panels: the inpainting strip has sf 1 (got sf " + std::to_string(d->sf) + ")"));
    if ((L_u8 || leh_u8) && !y) return fail(e, invalid("dpir_result_panels: an output needs y_dev"));
    if (leh_u8 && (!est || !gt)) return fail(e, invalid("dpir_result_panels: the strip needs est_u8_dev and gt_u8_dev"));
    const bool inset = kv && d->mode == 0;
    if (inset && (d->kh < 1 || d->kw < 1)) return fail(e, invalid("dpir_result_panels: kh and kw must be >= 1 with kernel bytes"));
    if (inset && (3LL * d->kh > d->H || 3LL * d->kw > d->W))
        return fail(e, invalid("dpir_result_panels: the x 3 kernel inset must fit the image, 3 kh <= H and 3 kw <= W (got kh " + std::to_string(d->kh) + ", kw " +
                               std::to_string(d->kw) + ", H " + std::to_string(d->H) + ", W " + std::to_string(d->W) + ")"));
    (void)hipSetDevice(e->device);
    ProfScope ps(&e->prof, PC_ELEM);
    ResultArgs a{y, inset ? kv : nullptr, est, gt, L_u8, leh_u8, d->B, d->H, d->W, d->sf, inset ? d->kh : 0, inset ? d->kw : 0, e->cus};
    API_TRY(e, launch_result_panels(e->stream, a));
    return DPIR_OK;
}

int dpir_lpips_load(dpir_engine* e, const dpir_tensor* weights, int n) {
    if (!e || !weights || n <= 0) return fail(e, invalid("dpir_lpips_load: null argument"));
    (void)hipSetDevice(e->device);
    API_TRY(e, lpips_load(e, weights, n));
    return DPIR_OK;
}

int dpir_lpips(dpir_engine* e, const float* x0, const uint8_t* gt_u8, const float* gt_f32, int B, int H, int W, float* lpips_host) {
    if (!e || !x0 || !lpips_host) return fail(e, invalid("dpir_lpips: null argument"));
    if ((gt_u8 != nullptr) == (gt_f32 != nullptr)) return fail(e, invalid("dpir_lpips: exactly one of gt_u8_dev and gt_f32_dev must be given"));
    API_TRY(e, check_shape("dpir_lpips", B, H, W));
    if (H < 16 || W < 16) return fail(e, invalid("dpir_lpips: H and W must be >= 16 (relu5_3 would be empty; got H " + std::to_string(H) + ", W " + std::to_string(W) + ")"));
    if (!e->lpips || !e->lpips->loaded) return fail(e, invalid("dpir_lpips: no LPIPS weights loaded (dpir_lpips_load)"));
    (void)hipSetDevice(e->device);
    {
        ProfScope ps(&e->prof, PC_ELEM);
        API_TRY(e, lpips_run(e, x0, gt_u8, gt_f32, B, H, W));
    }
    return dpir_d2h(e, lpips_host, e->lpips->score_f, sizeof(float) * B);
}

int dpir_lpips_keep_taps(dpir_engine* e, int on) {
    if (!e) return DPIR_ERR_INVALID;
    e->lpips_keep_taps = on != 0;
    return DPIR_OK;
}

int dpir_lpips_read_tap(dpir_engine* e, int k, float* host_dst, size_t cap, size_t* numel_out) {
    if (!e || !numel_out) return fail(e, invalid("dpir_lpips_read_tap: null argument"));
    if (k < 0 || k >= kLpipsTaps) return fail(e, invalid("dpir_lpips_read_tap: tap index must be 0..4"));
    if (!e->lpips || e->lpips->tap_numel[k] == 0) return fail(e, Status{DPIR_ERR_STATE, "dpir_lpips_read_tap: no kept taps (dpir_lpips_keep_taps before dpir_lpips)"});
    *numel_out = e->lpips->tap_numel[k];
    if (!host_dst) return DPIR_OK;
    if (cap < *numel_out) return fail(e, invalid("dpir_lpips_read_tap: destination too small"));
    return dpir_d2h(e, host_dst, e->lpips->tap[k], sizeof(float) * *numel_out);
}

int dpir_fid_load(dpir_engine* e, const dpir_tensor* weights, int n) {
    if (!e || !weights || n <= 0) return fail(e, invalid("dpir_fid_load: null argument"));
    (void)hipSetDevice(e->device);
    API_TRY(e, fid_load(e, weights, n));
    return DPIR_OK;
}

int dpir_fid_features(dpir_engine* e, const uint8_t* img_u8, const float* img_f32, int B, int H, int W, float* feat_host) {
    if (!e || !feat_host) return fail(e, invalid("dpir_fid_features: null argument"));
    if ((img_u8 != nullptr) == (img_f32 != nullptr)) return fail(e, invalid("dpir_fid_features: exactly one of img_u8_dev and img_f32_dev must be given"));
    API_TRY(e, check_shape("dpir_fid_features", B, H, W));
    if (!e->fid || !e->fid->loaded) return fail(e, Status{DPIR_ERR_STATE, "dpir_fid_features: no FID Inception weights loaded (dpir_fid_load)"});
    (void)hipSetDevice(e->device);
    {
        ProfScope ps(&e->prof, PC_ELEM);
        API_TRY(e, fid_run(e, img_u8, img_f32, B, H, W));
    }
    return dpir_d2h(e, feat_host, e->fid->feat, sizeof(float) * (size_t)B * kFidFeat);
}

int dpir_fid_keep_taps(dpir_engine* e, int on) {
    if (!e) return DPIR_ERR_INVALID;
    e->fid_keep_taps = on != 0;
    return DPIR_OK;
}

int dpir_fid_read_tap(dpir_engine* e, int k, float* host_dst, size_t cap, size_t* numel_out) {
    if (!e || !numel_out) return fail(e, invalid("dpir_fid_read_tap: null argument"));
    if (k < 0 || k >= kFidTaps) return fail(e, invalid("dpir_fid_read_tap: tap index must be 0..13"));
    if (!e->fid || e->fid->tap_numel[k] == 0)
        return fail(e, Status{DPIR_ERR_STATE, "dpir_fid_read_tap: nothing kept (dpir_fid_keep_taps before dpir_fid_features; tap 13, the features, needs only a call)"});
    *numel_out = e->fid->tap_numel[k];
    if (!host_dst) return DPIR_OK;
    if (cap < *numel_out) return fail(e, invalid("dpir_fid_read_tap: destination too small"));
    return dpir_d2h(e, host_dst, k == kFidTaps - 1 ? e->fid->feat : e->fid->tap[k], sizeof(float) * *numel_out);
}

}  // extern "C"

// ------------------------------------------------------------------------------------------ whole loop
// Every whole-loop runner is put together from the pieces of this section: loop_prologue (the shared refusals and buffers), film_table, loop_init,
// first_repaint_mix, denoise and loop_finish.  The three graph-capable runners (run_loop_once, run_inpaint_loop_once, run_ancestral_loop_once) hand their
// step to run_steps, the one place where a row becomes the current row and a step graph is looked up, captured or launched; run_grad_loop keeps an
// eager body of its own between loop_init and loop_finish.
namespace {
struct LoopBufs { int B, H, W; float *x, *x0, *out6, *n1, *n2, *init_src; int *t_dev, *y_dev; StepDev *steps_dev, *cur; LoopDev* lp;
                  float* film;      // film: hoisted FiLM table [n_steps][film_rows] (class-unconditional models) or null
                  // dpir_run_loop_per_image: the (tau, k1, k2, 0) table [n_steps][B] and the Philox image numbers [B] (both filled when per_image: a table
                  // the caller left out repeats the step's own scalars / image_offset + b); per_image selects the kernels' per-image instantiations
                  float4* img; long long* imgidx; bool per_image; };

__global__ void fill_t_kernel(int* p, const StepDev* sp, int n) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = sp->t;
}

// init (main_ddpir.py:291-320, main_ddpir_inpainting.py:190-193, main_ddpir_deblur.py:228-231): x_T = sa_start src + s1m_start n, both coefficients from
// the host.  What differs between the loops is passed in, not read from d.task (the gradient loop over the blur operator is task deblur and has neither
// spectra nor a mask): up_sf > 0 -- src is the bicubic up-sampling of y by up_sf (into b.init_src), 0 -- y itself; mask -- the known region keeps y
// (inpainting), or null; prox -- the spectra of the batch to pre-calculate, or null.
Status loop_init(dpir_engine* e, const dpir_loop_desc& d, const LoopBufs& b, int up_sf, const uint8_t* mask, ProxState* prox) {
    hipStream_t s = e->stream;
    const int B = d.B, H = d.H, W = d.W;
    const size_t total = (size_t)B * 3 * H * W;
    const float* src = d.y_dev;
    if (up_sf > 0) {
        ProfScope ps(&e->prof, PC_ELEM);
        DPIR_TRY(launch_bicubic_up(s, d.y_dev, b.init_src, B * 3, H / up_sf, W / up_sf, up_sf));   // main_ddpir.py:295
        src = b.init_src;
    }
    const float* n0 = d.noise_init_dev;
    if (!n0) { DPIR_TRY(launch_randn(s, b.n2, d.seed, 0, d.image_offset, B, (size_t)3 * H * W, nullptr, nullptr, b.per_image ? b.imgidx : nullptr)); n0 = b.n2; }
    {
        ProfScope ps(&e->prof, PC_ELEM);
        DPIR_TRY(launch_init_x(s, src, mask, n0, d.sa_start, d.s1m_start, b.x, total));
    }
    if (prox) DPIR_TRY(prox_precalc(e, d.y_dev, d.k_dev, d.kh, d.kw, prox));
    return Status{};
}

// The two fused loops, repaint: the first row's mix at its own noise level (main_ddpir_inpainting.py:244-246, main_ddpir.py:356-358); every later one
// is applied by the fused pass of the row before it
Status first_repaint_mix(dpir_engine* e, const dpir_loop_desc& d, const LoopBufs& b, float sa, float s1m) {
    ProfScope ps(&e->prof, PC_ELEM);
    const float* nr = d.noise_rp_dev;
    if (!nr) { DPIR_TRY(launch_randn(e->stream, b.n2, d.seed, 3, d.image_offset, b.B, (size_t)3 * b.H * b.W)); nr = b.n2; }
    return launch_repaint_mix(e->stream, b.x, d.y_dev, d.mask_dev, nr, sa, s1m, (size_t)b.B * 3 * b.H * b.W);
}

// The denoiser call of a graph-capable step: eps (and v) of b.x at the current row's timestep into b.out6.  cur_st is the StepDev at the head of the
// fixed-address current row; with the hoisted FiLM table the network reads its row from there, without it the timestep vector is filled from it
Status denoise(dpir_engine* e, const LoopBufs& b, const StepDev* cur_st) {
    if (!b.film) hipLaunchKernelGGL(fill_t_kernel, dim3((b.B + 255) / 256), dim3(256), 0, e->stream, b.t_dev, cur_st, b.B);
    return unet_forward(e, b.x, b.t_dev, b.y_dev, b.out6, b.B, b.H, b.W, b.film, b.film ? cur_st : nullptr);
}

// one iteration of main_ddpir.py:341-470; every per-step scalar is read on the device from b.cur
Status loop_step(dpir_engine* e, const dpir_loop_desc& d, const LoopBufs& b, ProxState* prox, bool last, bool with_n1) {
    hipStream_t s = e->stream;
    const int B = d.B, H = d.H, W = d.W;
    const size_t total = (size_t)B * 3 * H * W;
    if (d.generate_mode == 1) {          // repaint: re-draw the known region at the current noise level (main_ddpir.py:355-358)
        ProfScope ps(&e->prof, PC_ELEM);
        const float* nr = d.noise_rp_dev;
        size_t rstride = total;
        if (!nr) { DPIR_TRY(launch_randn(s, b.n1, d.seed, 3, d.image_offset, B, (size_t)3 * H * W, b.cur, b.lp, nullptr, b.per_image)); nr = b.n1; rstride = 0; }
        DPIR_TRY(launch_repaint_mix(s, b.x, d.y_dev, d.mask_dev, nr, 0.f, 0.f, total, b.cur, rstride, b.lp));
    }
    DPIR_TRY(denoise(e, b, b.cur));
    bool fused = false;      // the data step and the re-noise inside the prox's own three launches (half layouts): nothing is left to do here
    DPIR_TRY(prox_fused_step(e, *prox, d, last, with_n1, b.x, b.out6, b.x0, b.cur, b.lp, &fused, b.per_image));
    if (fused) return Status{};
    {
        ProfScope ps(&e->prof, PC_ELEM);
        DPIR_TRY(launch_xstart(s, b.x, b.out6, e->net.desc.out_channels, 0.f, 0.f, b.x0, B, H * W, b.cur));
    }
    if (last) return Status{};
    if (d.generate_mode != 0) {
        // repaint / vanilla: no data-fidelity step (main_ddpir.py:385 is DiffPIR only)
    } else if (d.first_order) {
        DPIR_TRY(prox_first_order_impl(e, b.x0, d.y_dev, 0.f, d.sf, B, H, W, b.cur, b.lp));
    } else if (d.task == DPIR_TASK_INPAINT) {
        ProfScope ps(&e->prof, PC_ELEM);
        DPIR_TRY(launch_prox_mask(s, b.x0, d.y_dev, d.mask_dev, 0.f, d.guidance, total, b.cur, b.lp, b.per_image));
    } else if (d.task == DPIR_TASK_SR_CUBIC) {
        DPIR_TRY(prox_ibp_impl(e, b.x0, d.y_dev, 0.f, d.gamma, d.in_iter, d.sf, B, H, W, b.cur, b.lp, b.per_image));
    } else {
        DPIR_TRY(prox_data_solution(e, *prox, b.x0, 0.5f, 0.5f, 1.f, b.x0, 2.f, -1.f, b.x0, d.guidance, b.cur, b.per_image ? b.lp : nullptr));
    }
    const float *n1 = nullptr, *n2 = nullptr;
    size_t stride = 0;
    ProfScope ps(&e->prof, PC_ELEM);
    if (with_n1) {
        if (d.noise_n1_dev) n1 = d.noise_n1_dev;
        else { DPIR_TRY(launch_randn(s, b.n1, d.seed, 1, d.image_offset, B, (size_t)3 * H * W, b.cur, b.lp, nullptr, b.per_image)); n1 = b.n1; }
    }
    if (d.noise_n2_dev) { n2 = d.noise_n2_dev; stride = total; }
    else { DPIR_TRY(launch_randn(s, b.n2, d.seed, 2, d.image_offset, B, (size_t)3 * H * W, b.cur, b.lp, nullptr, b.per_image)); n2 = b.n2; }
    if (with_n1 && d.noise_n1_dev && !d.noise_n2_dev) return invalid("host n1 noise requires host n2 noise");
    DPIR_TRY(launch_renoise(s, b.x, b.x0, RenoiseCoef{}, n1, n2, total, b.cur, stride, b.lp, b.per_image));
    DPIR_HIP(hipGetLastError());
    return Status{};
}
}  // namespace

extern "C" {

// Runs a whole-loop call and, in the f16 modes with the fused hop on, looks at the guard word afterwards: on a hop time-out the loop is run again
// on the unfused path.  Every graph-capable entry goes through it (dpir_run_loop, dpir_run_loop_per_image, dpir_run_inpaint_loop,
// dpir_run_ancestral_loop); the gradient loops do not (dpir_check_range reports a time-out inside them).
static int run_with_hop_guard(dpir_engine* e, const std::function<int()>& once) {
    int rc = once();
    static const bool fuse_env_off = getenv("DPIR_FUSE_H1") && atoi(getenv("DPIR_FUSE_H1")) == 0;       // unet.hip: the hop is not used at all
    if (rc != DPIR_OK || !e->range_ctr || e->precision == 0 || e->fuse_h1_off || fuse_env_off || e->grad_enabled) return rc;
    // the fused hop may have run: look at the guard word now (the caller synchronises right after the loop anyway) and, on a time-out,
    // run the whole loop again on the unfused path -- same inputs, same noise (device Philox is keyed by seed; host noise buffers are the caller's)
    unsigned long long n = 0;
    if (int r2 = read_range(e, &n)) return r2;
    e->fwd_since_sync = 0; e->replay_last = nullptr;
    if (!fuse_timeout_latch(e, n)) return DPIR_OK;      // plain range excursions stay in the counter for dpir_sync / dpir_d2h to report
    return once();
}

// The captured-step cache of the engine, shared by every graph-capable loop through run_steps (GraphKey::loop keeps their entries apart): the graph
// for `key` (ws_generation is filled in here), or -- on a miss -- `step` run eagerly once as a warm-up (every workspace buffer exists before capture;
// it is a real step of the loop, its result is kept: *ran = true), then captured and cached, evicting the least recently used entry but never
// `keep_a` / `keep_b` (the graphs the running loop already holds).
static int cached_step_graph(dpir_engine* e, dpir_engine::GraphKey key, const std::function<Status()>& step, hipGraphExec_t keep_a, hipGraphExec_t keep_b,
                             hipGraphExec_t* out, bool* ran) {
    *ran = false;
    key.ws_generation = e->ws.generation;
    for (auto& ge : e->graphs)
        if (memcmp(&ge.key, &key, sizeof(key)) == 0) { ge.last_use = ++e->graph_clock; *out = ge.exec; return DPIR_OK; }
    API_TRY(e, step());
    API_HIP(e, hipStreamSynchronize(e->stream));
    hipGraphExec_t exec = nullptr;
    API_TRY(e, capture_graph(e, step, &exec));
    if (e->graphs.size() >= dpir_engine::kMaxGraphs) {
        size_t lru = 0;
        for (size_t q = 1; q < e->graphs.size(); ++q) if (e->graphs[q].last_use < e->graphs[lru].last_use) lru = q;
        if (e->graphs[lru].exec == keep_a || e->graphs[lru].exec == keep_b) lru = (lru + 1) % e->graphs.size();
        (void)hipGraphExecDestroy(e->graphs[lru].exec);
        e->graphs.erase(e->graphs.begin() + lru);
    }
    key.ws_generation = e->ws.generation;       // the settled generation: the warm-up may have allocated
    dpir_engine::GraphEntry ge; ge.key = key; ge.exec = exec; ge.last_use = ++e->graph_clock;
    e->graphs.push_back(ge);
    *out = exec; *ran = true;
    return DPIR_OK;
}

// What a whole-loop runner tells loop_prologue about itself
struct LoopCall {
    const char* entry;                      // the public entry's name: the prefix of the refusals
    int n; const char* noun;                // length of the step / row table, and what the entry calls one of its entries
    std::vector<char> last;                 // the table's `last` flags (empty: the table has none)
    int mode_lo = 0;                        // generate_mode must lie in mode_lo .. 2 and is refused as "generate_mode must be <modes>";
    const char* modes = "0 (DiffPIR), 1 (repaint) or 2 (vanilla)";      // null: not read (the gradient loops are told their variant)
    bool x0 = false, n1 = false, init = false, t = false;      // the workspace buffers of LoopBufs it uses besides x, out6, n2 and the labels
    Status own;                             // the entry's own refusal (task, shape, variant, host noise): reported after "no model", ahead of the shared ones
};

// The head of every whole-loop runner: what all of them refuse, then -- nothing is enqueued or allocated before this point -- a new range accounting
// period, the workspace images and the labels.  (A workspace request past this point still precedes every capture: see run_steps.)
static int loop_prologue(dpir_engine* e, const LoopCall& c, const dpir_loop_desc& d, LoopBufs* b) {
    (void)hipSetDevice(e->device);
    const std::string entry = c.entry;
    if (!e->net.loaded) return fail(e, Status{DPIR_ERR_STATE, "dpir_load_unet has not been called"});
    API_TRY(e, c.own);
    if (c.modes && (d.generate_mode < c.mode_lo || d.generate_mode > 2)) return fail(e, invalid(entry + ": generate_mode must be " + c.modes));
    API_TRY(e, labels_match(e, d.labels_host));
    // the reference marks EVERY step with seq[i] == seq[-1] as final (two of them for quad skipping with iter_num > T/2): each is a dead
    // denoiser call, prox and re-noise are skipped (main_ddpir.py:384, 448)
    for (size_t i = 1; i < c.last.size(); ++i)
        if (c.last[i - 1] && !c.last[i]) return fail(e, invalid(entry + ": a non-final " + c.noun + " may not follow a final " + c.noun));
    API_TRY(e, progress_check(e, c.entry, c.n, d));
    range_clear(e);
    const size_t total = (size_t)d.B * 3 * d.H * d.W;
    b->B = d.B; b->H = d.H; b->W = d.W;
    API_TRY(e, e->ws.getT("loop#x", total, &b->x));
    if (c.x0) API_TRY(e, e->ws.getT("loop#x0", total, &b->x0));
    API_TRY(e, e->ws.getT("loop#out6", (size_t)d.B * e->net.desc.out_channels * d.H * d.W, &b->out6));
    if (c.n1) API_TRY(e, e->ws.getT("loop#n1", total, &b->n1));
    API_TRY(e, e->ws.getT("loop#n2", total, &b->n2));
    if (c.init) API_TRY(e, e->ws.getT("loop#init", total, &b->init_src));
    if (c.t) API_TRY(e, e->ws.getT("loop#t", (size_t)d.B, &b->t_dev));
    API_TRY(e, upload_ints(e, "loop#y", d.labels_host, d.B, &b->y_dev));
    return DPIR_OK;
}

// Time embedding + every ResBlock's FiLM projection for the timesteps ts, once per call (class-unconditional models: the timestep is batch-uniform).
// Row i of the table serves the steps / rows whose StepDev::i is i.  *film stays null for a class-conditional model.
static Status film_table(dpir_engine* e, const std::vector<int64_t>& ts, float** film) {
    if (e->net.desc.num_classes != 0) return Status{};
    const int n = (int)ts.size();
    int* ts_dev = nullptr;
    DPIR_TRY(e->ws.getT("loop#film", (size_t)n * e->net.film_rows, film));
    DPIR_TRY(upload_ints(e, "loop#ts", ts.data(), n, &ts_dev));
    return unet_film_table(e, ts_dev, n, *film);
}

// Repaint with a progress strip armed: the fused pass of the two fused loops mixes the next row's known region into x before x ever reaches memory,
// so the rows that own a panel also write the pre-mix x to this scratch image, which the snapshot then reads.  (The alternative, forming the panel
// inside the fused pass, would put the strip layout, the uint8 / masked outputs and the min/max reduction into that kernel a second time.)
// A plain allocation, not a workspace buffer: see dpir_engine::progress_premix.
static Status ensure_premix(dpir_engine* e, size_t total) {
    if (e->progress_premix_bytes >= total * sizeof(float)) return Status{};
    DPIR_HIP(hipStreamSynchronize(e->stream));
    if (e->progress_premix) (void)hipFree(e->progress_premix);
    e->progress_premix = nullptr; e->progress_premix_bytes = 0;
    DPIR_HIP(hipMalloc((void**)&e->progress_premix, total * sizeof(float)));
    e->progress_premix_bytes = total * sizeof(float);
    return Status{};
}

// The tail of every whole-loop runner: the last entry's panel (read from panel_x) and x -> the caller's output
static int loop_finish(dpir_engine* e, const dpir_loop_desc& d, const LoopBufs& b, int n, const float* panel_x, float* out_f32, uint8_t* out_u8) {
    API_TRY(e, progress_emit(e, n - 1, panel_x, d));
    ProfScope ps(&e->prof, PC_ELEM);
    API_TRY(e, launch_finalize(e->stream, b.x, out_f32, out_u8, d.B, d.H * d.W));
    return DPIR_OK;
}

// What a graph-capable loop hands to run_steps.  A row is classified as ROW_SKIP (nothing runs), ROW_DATA_ONLY (data_pass alone) or the graph slot
// whose step runs it: dpir_run_loop has two (0 the ordinary step, 1 the final step), the fused loops one.
enum { ROW_SKIP = -2, ROW_DATA_ONLY = -1 };
struct StepLoop {
    int n;                                                  // rows
    const void* rows_dev; void* cur; size_t row_bytes;      // the device table and the fixed-address current row its steps read
    std::function<int(int)> slot_of;                        // row -> ROW_SKIP | ROW_DATA_ONLY | slot
    std::function<Status(int)> step;                        // slot -> the step: run eagerly, or recorded into the slot's graph
    std::function<Status()> data_pass;                      // ROW_DATA_ONLY rows (only a loop that classifies one so sets it)
    std::function<dpir_engine::GraphKey(int)> key_of;       // slot -> everything baked into its graph but the workspace generation
    std::function<const float*(int)> panel_x;               // row -> the image its progress panel is read from once the row has run
};

// The step driver of the graph-capable loops.  Row i: the panel of row i - 1 first (a panel shows x after its row, and is taken when the next row
// begins, or in loop_finish, so that a row skipped as dead yields its panel too); then the row's class; row i -> the current row; the step, eagerly
// or as a graph.  One graph per slot serves all rows: a slot's first row looks it up in the engine's cache or, on a miss, IS the warm-up that
// cached_step_graph runs eagerly before capturing.  No workspace request may fall between a capture and its replay: all of them precede this call
// or happen inside the warm-up step.
static int run_steps(dpir_engine* e, const dpir_loop_desc& d, const LoopBufs& b, const StepLoop& L, float* out_f32, uint8_t* out_u8) {
    hipGraphExec_t g[2] = {nullptr, nullptr};
    for (int i = 0; i < L.n; ++i) {
        if (i > 0) API_TRY(e, progress_emit(e, i - 1, L.panel_x(i - 1), d));
        const int slot = L.slot_of(i);
        if (slot == ROW_SKIP) continue;
        API_HIP(e, hipMemcpyAsync(L.cur, static_cast<const char*>(L.rows_dev) + (size_t)i * L.row_bytes, L.row_bytes, hipMemcpyDeviceToDevice, e->stream));
        if (slot == ROW_DATA_ONLY) { API_TRY(e, L.data_pass()); continue; }
        if (!d.use_graph) { API_TRY(e, L.step(slot)); continue; }
        if (!g[slot]) {
            bool ran = false;
            if (int rc = cached_step_graph(e, L.key_of(slot), [&] { return L.step(slot); }, g[0], g[1], &g[slot], &ran)) return rc;
            if (ran) continue;   // this row was executed eagerly
        }
        ProfScope ps(&e->prof, PC_LOOP);
        API_HIP(e, hipGraphLaunch(g[slot], e->stream));
    }
    return loop_finish(e, d, b, L.n, L.panel_x(L.n - 1), out_f32, out_u8);
}

static int run_loop_once(dpir_engine* e, const dpir_loop_desc* dd, const dpir_step* steps, int n_steps, const dpir_image_step* per_image,
                         const int64_t* image_index, float* out_f32, uint8_t* out_u8) {
    if (!e || !dd || !steps || n_steps <= 0) return fail(e, invalid("dpir_run_loop: null argument"));
    const dpir_loop_desc& d = *dd;
    const bool need_prox = d.task == DPIR_TASK_DEBLUR || d.task == DPIR_TASK_SR_BLUR;
    bool with_n1 = false;
    LoopCall c{"dpir_run_loop", n_steps, "step", std::vector<char>(n_steps)};
    c.x0 = c.n1 = c.init = c.t = true;
    for (int i = 0; i < n_steps; ++i) {
        c.last[i] = steps[i].last != 0;
        if (!steps[i].last && steps[i].es != 0.f) with_n1 = true;
    }
    c.own = [&]() -> Status {
        if (d.B <= 0 || d.H <= 0 || d.W <= 0 || d.sf < 1 || d.H % d.sf || d.W % d.sf) return invalid("dpir_run_loop: bad shape");
        if (!d.y_dev) return invalid("dpir_run_loop: y is required");
        if (need_prox && !d.k_dev) return invalid("dpir_run_loop: task needs a PSF");
        if (d.task == DPIR_TASK_INPAINT && !d.mask_dev) return invalid("dpir_run_loop: inpainting needs a mask");
        if (d.task < 0 || d.task > 3) return invalid("dpir_run_loop: unknown task");
        if (d.generate_mode != 0 && d.task != DPIR_TASK_INPAINT)
            return invalid("dpir_run_loop: repaint / vanilla are inpainting modes (main_ddpir.py:448 re-noises only for inpainting or DiffPIR)");
        if (d.first_order && (d.generate_mode != 0 || (d.task != DPIR_TASK_SR_BLUR && d.task != DPIR_TASK_SR_CUBIC)))
            return Status{DPIR_ERR_UNSUPPORTED, "the first-order data step (sub_1_analytic: false) is implemented for the DiffPIR mode of the "
                                                "super-resolution tasks (the reference's deblurring operator raises at main_ddpir.py:302)"};
        if (with_n1 && d.noise_n2_dev && !d.noise_n1_dev) return invalid("dpir_run_loop: eta != 0 with host noise needs noise_n1_dev");
        return Status{};
    }();
    LoopBufs b{};
    if (int rc = loop_prologue(e, c, d, &b)) return rc;
    const int B = d.B, H = d.H, W = d.W;
    API_TRY(e, e->ws.getT("loop#steps", (size_t)n_steps, &b.steps_dev));
    API_TRY(e, e->ws.getT("loop#cur", (size_t)1, &b.cur));
    API_TRY(e, e->ws.getT("loop#lp", (size_t)1, &b.lp));
    // the per-image tables are workspace buffers of EVERY call (a uniform one leaves them unwritten): were they allocated by the first per-image call, the
    // workspace generation would move and orphan the uniform steps already captured
    API_TRY(e, e->ws.getT("loop#img", (size_t)n_steps * B, &b.img));
    API_TRY(e, e->ws.getT("loop#imgidx", (size_t)B, &b.imgidx));
    b.per_image = per_image != nullptr || image_index != nullptr;
    std::vector<int64_t> ts(n_steps);
    for (int i = 0; i < n_steps; ++i) ts[i] = steps[i].t;
    API_TRY(e, film_table(e, ts, &b.film));
    ProxState& prox = e->loop_prox;
    if (need_prox) {
        bool reallocated = false;
        const Status ps = prox_ensure(e, d.sf, B, H, W, &prox, &reallocated);
        if (reallocated) {        // the captured steps hold the addresses of the spectra that went
            API_HIP(e, hipStreamSynchronize(e->stream));
            e->invalidate_graphs();
        }
        API_TRY(e, ps);
    }

    // per-step scalar table and the per-batch device block -> device (two small H2D copies per batch)
    {
        std::vector<StepDev> hs(n_steps);
        for (int i = 0; i < n_steps; ++i) {
            const dpir_step& st = steps[i];
            hs[i] = StepDev{st.t, st.last, i, 0, st.c1, st.c2, st.tau, st.sa_t, st.s1m_t, st.sa_p, st.k1, st.q, st.es, st.k2};
        }
        LoopDev hl{d.y_dev, d.mask_dev, d.noise_n1_dev, d.noise_n2_dev, d.noise_rp_dev, (unsigned long long)d.seed, (long long)d.image_offset,
                   b.per_image ? b.img : nullptr, b.per_image ? b.imgidx : nullptr, B, 0};
        std::vector<float4> himg;
        std::vector<long long> hidx;
        if (b.per_image) {
            himg.resize((size_t)n_steps * B);
            for (int i = 0; i < n_steps; ++i)
                for (int n = 0; n < B; ++n) {
                    const dpir_image_step* r = per_image ? per_image + (size_t)i * B + n : nullptr;
                    himg[(size_t)i * B + n] = r ? make_float4(r->tau, r->k1, r->k2, 0.f) : make_float4(steps[i].tau, steps[i].k1, steps[i].k2, 0.f);
                }
            hidx.resize(B);
            for (int n = 0; n < B; ++n) hidx[n] = image_index ? (long long)image_index[n] : (long long)d.image_offset + n;
            API_HIP(e, hipMemcpyAsync(b.img, himg.data(), sizeof(float4) * himg.size(), hipMemcpyHostToDevice, e->stream));
            API_HIP(e, hipMemcpyAsync(b.imgidx, hidx.data(), sizeof(long long) * B, hipMemcpyHostToDevice, e->stream));
        }
        API_HIP(e, hipMemcpyAsync(b.steps_dev, hs.data(), sizeof(StepDev) * n_steps, hipMemcpyHostToDevice, e->stream));
        API_HIP(e, hipMemcpyAsync(b.lp, &hl, sizeof(hl), hipMemcpyHostToDevice, e->stream));
        API_HIP(e, hipStreamSynchronize(e->stream));
    }
    const bool sr = d.task == DPIR_TASK_SR_BLUR || d.task == DPIR_TASK_SR_CUBIC;
    API_TRY(e, loop_init(e, d, b, sr ? d.sf : 0, d.task == DPIR_TASK_INPAINT ? d.mask_dev : nullptr, need_prox ? &prox : nullptr));

    StepLoop L{n_steps, b.steps_dev, b.cur, sizeof(StepDev)};
    // the repaint mix of this loop opens the NEXT step, so every panel is x itself; skip_dead_final_eval drops the dead final step(s) altogether
    L.panel_x = [&](int) { return b.x; };
    L.slot_of = [&](int i) { return !steps[i].last ? 0 : d.skip_dead_final_eval ? (int)ROW_SKIP : 1; };
    L.step = [&](int slot) { return loop_step(e, d, b, &prox, slot == 1, with_n1); };
    L.key_of = [&](int slot) {
        dpir_engine::GraphKey k{};
        k.task = d.task; k.B = B; k.H = H; k.W = W; k.sf = d.sf; k.in_iter = d.in_iter; k.generate_mode = d.generate_mode;
        k.kind = (slot == 1 ? 1 : 0) | (with_n1 ? 2 : 0) | (d.first_order ? 4 : 0);
        k.host_n1 = d.noise_n1_dev != nullptr; k.host_n2 = d.noise_n2_dev != nullptr; k.host_rp = d.noise_rp_dev != nullptr;
        k.has_labels = d.labels_host != nullptr;
        k.gamma = d.gamma; k.guidance = d.guidance;
        k.per_image = per_image != nullptr; k.image_index = image_index != nullptr;
        return k;
    };
    return run_steps(e, d, b, L, out_f32, out_u8);
}

int dpir_run_loop(dpir_engine* e, const dpir_loop_desc* dd, const dpir_step* steps, int n_steps, float* out_f32, uint8_t* out_u8) {
    ProgressOneShot one_shot{e};
    return run_with_hop_guard(e, [&] { return run_loop_once(e, dd, steps, n_steps, nullptr, nullptr, out_f32, out_u8); });
}
int dpir_run_loop_per_image(dpir_engine* e, const dpir_loop_desc* dd, const dpir_step* steps, int n_steps, const dpir_image_step* per_image,
                            const int64_t* image_index, float* out_f32, uint8_t* out_u8) {
    ProgressOneShot one_shot{e};
    // refused before anything is enqueued: the first-order data step normalises by ONE residual norm of the whole batch (main_ddpir.py:425-427)
    if (e && dd && per_image && dd->first_order)
        return fail(e, Status{DPIR_ERR_UNSUPPORTED, "dpir_run_loop_per_image: the first-order data step (sub_1_analytic: false) has no per-image form: it "
                                                    "normalises by a batch-wide residual norm"});
    return run_with_hop_guard(e, [&] { return run_loop_once(e, dd, steps, n_steps, per_image, image_index, out_f32, out_u8); });
}

// ------------------------------------------------------------------------------------------ inpainting with resampling (main_ddpir_inpainting.py)
static InpaintRowDev row_dev_of(const dpir_inpaint_row& r, int s) {
    InpaintRowDev o{};
    o.st = StepDev{r.t, r.last, r.pos, 0, r.c1, r.c2, r.tau, r.sa_t, r.s1m_t, r.sa_p, r.k1, r.q, r.es, r.k2};
    o.s = s; o.back = r.back; o.mix_next = r.mix_next; o.emit = 0;
    o.sae = r.sae; o.sb = r.sb; o.sa_n = r.sa_n; o.s1m_n = r.s1m_n;
    return o;
}

int dpir_inpaint_step(dpir_engine* e, float* x, const float* eps, int eps_ch, const float* y, const uint8_t* mask, const dpir_inpaint_row* row,
                      int generate_mode, float guidance, const float* n1, const float* n2, const float* n_back, const float* n_rp_next,
                      uint64_t seed, int64_t image_offset, int substep, float* x0_out, int B, int H, int W) {
    if (!e || !x || !eps || !y || !mask || !row) return fail(e, invalid("dpir_inpaint_step: null argument"));
    API_TRY(e, check_shape("dpir_inpaint_step", B, H, W));
    if (eps_ch != 3 && eps_ch != 6) return fail(e, invalid("dpir_inpaint_step: eps_channels must be 3 or 6"));
    if (generate_mode < 0 || generate_mode > 2) return fail(e, invalid("dpir_inpaint_step: generate_mode must be 0 (DiffPIR), 1 (repaint) or 2 (vanilla)"));
    if (substep < 0) return fail(e, invalid("dpir_inpaint_step: substep must be >= 0"));
    const bool host = n2 != nullptr;
    if (!host && (n1 || n_back || n_rp_next)) return fail(e, invalid("dpir_inpaint_step: host noise needs n2 (all four null selects device noise)"));
    if (host && !row->last) {
        if (row->es != 0.f && !n1) return fail(e, invalid("dpir_inpaint_step: eta_sigma != 0 needs n1"));
        if (row->back && !n_back) return fail(e, invalid("dpir_inpaint_step: a set-back row needs n_back"));
    }
    if (host && generate_mode == 1 && row->mix_next && !n_rp_next) return fail(e, invalid("dpir_inpaint_step: the repaint mix needs n_repaint_next"));
    (void)hipSetDevice(e->device);
    ProfScope ps(&e->prof, PC_ELEM);
    InpaintStepArgs a{};
    a.x = x; a.eps = eps; a.eps_ch = eps_ch; a.y = y; a.mask = mask; a.mode = generate_mode; a.guidance = guidance;
    a.device_noise = host ? 0 : 1; a.n1 = n1; a.n2 = n2; a.nback = n_back; a.nrp_next = n_rp_next;
    a.seed = seed; a.image_offset = image_offset; a.x0_out = x0_out; a.row = nullptr; a.row_val = row_dev_of(*row, substep); a.lp = nullptr; a.B = B; a.HW = H * W; a.cus = e->cus;
    API_TRY(e, launch_inpaint_step(e->stream, a));
    return DPIR_OK;
}

static int run_inpaint_loop_once(dpir_engine* e, const dpir_loop_desc* dd, const dpir_inpaint_row* rows, int n_rows, const float* noise_back,
                                 float* out_f32, uint8_t* out_u8) {
    if (!e || !dd || !rows || n_rows <= 0) return fail(e, invalid("dpir_run_inpaint_loop: null argument"));
    const dpir_loop_desc& d = *dd;
    const bool host = d.noise_n2_dev != nullptr;
    LoopCall c{"dpir_run_inpaint_loop", n_rows, "row", std::vector<char>(n_rows)};
    c.t = true;
    for (int r = 0; r < n_rows; ++r) c.last[r] = rows[r].last != 0;
    c.own = [&]() -> Status {
        DPIR_TRY(check_shape("dpir_run_inpaint_loop", d.B, d.H, d.W));
        if (d.task != DPIR_TASK_INPAINT || d.sf != 1) return invalid("dpir_run_inpaint_loop: the standalone inpainting program's loop: task must be inpainting, sf 1");
        if (!d.y_dev || !d.mask_dev) return invalid("dpir_run_inpaint_loop: y and mask are required");
        if (d.first_order) return Status{DPIR_ERR_UNSUPPORTED, "sub_1_analytic: false is a TODO in the reference (main_ddpir_inpainting.py:280-283)"};
        bool with_n1 = false, any_back = false;
        for (int r = 0; r < n_rows; ++r) {
            const dpir_inpaint_row& w = rows[r];
            if (!w.last && w.es != 0.f) with_n1 = true;
            if (!w.last && w.back) any_back = true;
            if (w.pos < 0 || w.pos >= n_rows || (r > 0 && (w.pos < rows[r - 1].pos || w.pos > rows[r - 1].pos + 1)) || (r == 0 && w.pos != 0))
                return invalid("dpir_run_inpaint_loop: pos must start at 0 and grow by 0 or 1 per row");
            if ((w.mix_next != 0) != (r + 1 < n_rows)) return invalid("dpir_run_inpaint_loop: mix_next must be 1 on every row but the last");
        }
        if (host) {
            if (!d.noise_init_dev) return invalid("dpir_run_inpaint_loop: host noise needs noise_init_dev");
            if (with_n1 && !d.noise_n1_dev) return invalid("dpir_run_inpaint_loop: eta != 0 with host noise needs noise_n1_dev");
            if (any_back && !noise_back) return invalid("dpir_run_inpaint_loop: iter_num_U > 1 with host noise needs noise_back_dev");
            if (d.generate_mode == 1 && !d.noise_rp_dev) return invalid("dpir_run_inpaint_loop: repaint with host noise needs noise_rp_dev");
        } else if (d.noise_init_dev || d.noise_n1_dev || d.noise_rp_dev || noise_back) {
            return invalid("dpir_run_inpaint_loop: host noise needs noise_n2_dev (all null selects device noise)");
        }
        return Status{};
    }();
    LoopBufs b{};
    if (int rc = loop_prologue(e, c, d, &b)) return rc;
    const int B = d.B, H = d.H, W = d.W;
    const dpir_engine::Progress& pg = e->progress;
    const bool premix = pg.armed && d.generate_mode == 1;
    if (premix) API_TRY(e, ensure_premix(e, (size_t)B * 3 * H * W));
    InpaintRowDev *rows_dev = nullptr, *cur = nullptr;
    InpaintLoopDev* lp = nullptr;
    API_TRY(e, e->ws.getT("inpaint#rows", (size_t)n_rows, &rows_dev));
    API_TRY(e, e->ws.getT("inpaint#cur", (size_t)1, &cur));
    API_TRY(e, e->ws.getT("inpaint#lp", (size_t)1, &lp));
    std::vector<int64_t> ts(rows[n_rows - 1].pos + 1);      // one FiLM row per visited timestep: the U sub-steps of a timestep share it (row.pos)
    {
        std::vector<InpaintRowDev> hr(n_rows);
        for (int r = 0; r < n_rows; ++r) { hr[r] = row_dev_of(rows[r], r); hr[r].emit = premix && pg.panel_of[r] >= 0; ts[rows[r].pos] = rows[r].t; }
        InpaintLoopDev hl{d.y_dev, d.mask_dev, d.noise_n1_dev, d.noise_n2_dev, noise_back, d.noise_rp_dev, (unsigned long long)d.seed, (long long)d.image_offset,
                          premix ? e->progress_premix : nullptr};
        API_HIP(e, hipMemcpyAsync(rows_dev, hr.data(), sizeof(InpaintRowDev) * n_rows, hipMemcpyHostToDevice, e->stream));
        API_HIP(e, hipMemcpyAsync(lp, &hl, sizeof(hl), hipMemcpyHostToDevice, e->stream));
        API_HIP(e, hipStreamSynchronize(e->stream));
    }
    API_TRY(e, film_table(e, ts, &b.film));
    API_TRY(e, loop_init(e, d, b, 0, d.mask_dev, nullptr));      // x from y's own noise level: sa_start / s1m_start (main_ddpir_inpainting.py:190-193)
    if (d.generate_mode == 1) API_TRY(e, first_repaint_mix(e, d, b, rows[0].sa_t, rows[0].s1m_t));
    // one 16-byte access per lane needs every tensor behind lp aligned; the decision is baked into a captured graph, so it is part of its key
    const bool aligned = aligned16(d.y_dev) && aligned4(d.mask_dev) && aligned16(d.noise_n1_dev) && aligned16(d.noise_n2_dev) && aligned16(noise_back) &&
                         aligned16(d.noise_rp_dev);
    InpaintStepArgs a{};
    a.x = b.x; a.eps = b.out6; a.eps_ch = e->net.desc.out_channels; a.mode = d.generate_mode; a.guidance = d.guidance;
    a.device_noise = host ? 0 : 1; a.row = cur; a.lp = lp; a.B = B; a.HW = H * W; a.cus = e->cus; a.scalar_only = aligned ? 0 : 1;

    StepLoop L{n_rows, rows_dev, cur, sizeof(InpaintRowDev)};
    // repaint: a row that mixed the next one in left its own x in the scratch image
    L.panel_x = [&](int r) { return premix && rows[r].mix_next ? e->progress_premix : b.x; };
    // the dead final evaluation is skipped, the next row's mix is not: it reaches x_0
    L.slot_of = [&](int r) { return !(rows[r].last && d.skip_dead_final_eval) ? 0 : d.generate_mode == 1 && rows[r].mix_next ? (int)ROW_DATA_ONLY : (int)ROW_SKIP; };
    L.data_pass = [&]() -> Status {
        ProfScope ps(&e->prof, PC_ELEM);
        return launch_inpaint_step(e->stream, a);
    };
    L.step = [&](int) -> Status {
        DPIR_TRY(denoise(e, b, &cur->st));
        return L.data_pass();
    };
    L.key_of = [&](int) {
        dpir_engine::GraphKey k{};
        k.task = d.task; k.B = B; k.H = H; k.W = W; k.sf = 1; k.generate_mode = d.generate_mode;
        k.kind = aligned ? 1 : 0;
        k.host_n1 = d.noise_n1_dev != nullptr; k.host_n2 = host; k.host_rp = d.noise_rp_dev != nullptr;
        k.has_labels = d.labels_host != nullptr;
        k.guidance = d.guidance; k.loop = 1;
        return k;
    };
    return run_steps(e, d, b, L, out_f32, out_u8);
}

int dpir_run_inpaint_loop(dpir_engine* e, const dpir_loop_desc* dd, const dpir_inpaint_row* rows, int n_rows, const float* noise_back,
                          float* out_f32, uint8_t* out_u8) {
    ProgressOneShot one_shot{e};
    return run_with_hop_guard(e, [&] { return run_inpaint_loop_once(e, dd, rows, n_rows, noise_back, out_f32, out_u8); });
}

// ------------------------------------------------------------------------------------------ ancestral inpainting loops (main_ddpir.py, 'pred_x_prev')
static AncestralRowDev ancestral_row_dev_of(const dpir_ancestral_row& r, int s) {
    AncestralRowDev o{};
    o.st = StepDev{r.t, 0, s, 0, r.c1, r.c2, 0.f, r.sa_t, r.s1m_t, 0.f, 0.f, 0.f, 0.f, 0.f};
    o.s = s; o.nonzero = r.nonzero; o.mix_next = r.mix_next; o.emit = 0;
    o.pc1 = r.pc1; o.pc2 = r.pc2; o.min_log = r.min_log; o.max_log = r.max_log;
    o.sa_prev = r.sa_prev; o.s1m_prev = r.s1m_prev; o.sa_n = r.sa_n; o.s1m_n = r.s1m_n;
    return o;
}

static const char* kNeedsLearnSigma = "p_sample needs a learn_sigma model (out_channels == 6): the learned-range variance is read from channels 3..5";

int dpir_ancestral_step(dpir_engine* e, float* x, const float* out6, int out_ch, const float* y, const uint8_t* mask, const dpir_ancestral_row* row,
                        int generate_mode, int ddim, const float* n_ps, const float* n_rp_next, uint64_t seed, int64_t image_offset, int step,
                        float* x0_out, int B, int H, int W) {
    if (!e || !x || !out6 || !row) return fail(e, invalid("dpir_ancestral_step: null argument"));
    API_TRY(e, check_shape("dpir_ancestral_step", B, H, W));
    if (generate_mode != 1 && generate_mode != 2) return fail(e, invalid("dpir_ancestral_step: generate_mode must be 1 (repaint) or 2 (vanilla)"));
    if (generate_mode == 1 && (!y || !mask)) return fail(e, invalid("dpir_ancestral_step: repaint needs y and mask"));
    if (step < 0) return fail(e, invalid("dpir_ancestral_step: step must be >= 0"));
    const bool host = n_ps != nullptr;
    if (!host && n_rp_next) return fail(e, invalid("dpir_ancestral_step: host noise needs n_ps (both null selects device noise)"));
    if (host && generate_mode == 1 && row->mix_next && !n_rp_next) return fail(e, invalid("dpir_ancestral_step: the repaint mix needs n_repaint_next"));
    if (out_ch != 6) return fail(e, Status{DPIR_ERR_UNSUPPORTED, std::string("dpir_ancestral_step: ") + kNeedsLearnSigma});
    (void)hipSetDevice(e->device);
    ProfScope ps(&e->prof, PC_ELEM);
    AncestralStepArgs a{};
    a.x = x; a.out6 = out6; a.y = y; a.mask = mask; a.mode = generate_mode; a.ddim = ddim ? 1 : 0;
    a.device_noise = host ? 0 : 1; a.nps = n_ps; a.nrp_next = n_rp_next;
    a.seed = seed; a.image_offset = image_offset; a.x0_out = x0_out; a.row = nullptr; a.row_val = ancestral_row_dev_of(*row, step); a.lp = nullptr;
    a.B = B; a.HW = H * W; a.cus = e->cus;
    API_TRY(e, launch_ancestral_step(e->stream, a));
    return DPIR_OK;
}

static int run_ancestral_loop_once(dpir_engine* e, const dpir_loop_desc* dd, const dpir_ancestral_row* rows, int n_rows, const float* noise_ps,
                                   float* out_f32, uint8_t* out_u8) {
    if (!e || !dd || !rows || n_rows <= 0) return fail(e, invalid("dpir_run_ancestral_loop: null argument"));
    const dpir_loop_desc& d = *dd;
    const bool host = noise_ps != nullptr;
    const bool repaint = d.generate_mode == 1;
    LoopCall c{"dpir_run_ancestral_loop", n_rows, "row", {}};       // no row is final: the loop has no dead step
    c.mode_lo = 1; c.modes = "1 (repaint) or 2 (vanilla); DiffPIR with pred_x_prev reads an unbound tau at main_ddpir.py:417";
    c.t = true;
    c.own = [&]() -> Status {
        DPIR_TRY(check_shape("dpir_run_ancestral_loop", d.B, d.H, d.W));
        if (d.task != DPIR_TASK_INPAINT || d.sf != 1)
            return invalid("dpir_run_ancestral_loop: task must be inpainting, sf 1 (main_ddpir.py:355-366 updates x from 'pred_x_prev' for inpainting only)");
        if (!d.y_dev || !d.mask_dev) return invalid("dpir_run_ancestral_loop: y and mask are required");
        if (e->net.desc.out_channels != 6) return Status{DPIR_ERR_UNSUPPORTED, std::string("dpir_run_ancestral_loop: ") + kNeedsLearnSigma};
        for (int r = 0; r < n_rows; ++r)
            if ((rows[r].mix_next != 0) != (r + 1 < n_rows)) return invalid("dpir_run_ancestral_loop: mix_next must be 1 on every row but the last");
        if (host) {
            if (!d.noise_init_dev) return invalid("dpir_run_ancestral_loop: host noise needs noise_init_dev");
            if (repaint && !d.noise_rp_dev) return invalid("dpir_run_ancestral_loop: repaint with host noise needs noise_rp_dev");
        } else if (d.noise_init_dev || d.noise_rp_dev) {
            return invalid("dpir_run_ancestral_loop: host noise needs noise_ps_dev (all null selects device noise)");
        }
        return Status{};
    }();
    LoopBufs b{};
    if (int rc = loop_prologue(e, c, d, &b)) return rc;
    const int B = d.B, H = d.H, W = d.W;
    const dpir_engine::Progress& pg = e->progress;
    const bool premix = pg.armed && repaint;
    if (premix) API_TRY(e, ensure_premix(e, (size_t)B * 3 * H * W));
    AncestralRowDev *rows_dev = nullptr, *cur = nullptr;
    AncestralLoopDev* lp = nullptr;
    API_TRY(e, e->ws.getT("ancestral#rows", (size_t)n_rows, &rows_dev));
    API_TRY(e, e->ws.getT("ancestral#cur", (size_t)1, &cur));
    API_TRY(e, e->ws.getT("ancestral#lp", (size_t)1, &lp));
    std::vector<int64_t> ts(n_rows);        // one FiLM row per step
    {
        std::vector<AncestralRowDev> hr(n_rows);
        for (int r = 0; r < n_rows; ++r) { hr[r] = ancestral_row_dev_of(rows[r], r); hr[r].emit = premix && pg.panel_of[r] >= 0; ts[r] = rows[r].t; }
        AncestralLoopDev hl{d.y_dev, d.mask_dev, noise_ps, d.noise_rp_dev, (unsigned long long)d.seed, (long long)d.image_offset,
                            premix ? e->progress_premix : nullptr};
        API_HIP(e, hipMemcpyAsync(rows_dev, hr.data(), sizeof(AncestralRowDev) * n_rows, hipMemcpyHostToDevice, e->stream));
        API_HIP(e, hipMemcpyAsync(lp, &hl, sizeof(hl), hipMemcpyHostToDevice, e->stream));
        API_HIP(e, hipStreamSynchronize(e->stream));
    }
    API_TRY(e, film_table(e, ts, &b.film));
    API_TRY(e, loop_init(e, d, b, 0, d.mask_dev, nullptr));      // main_ddpir.py:312-315
    if (repaint) API_TRY(e, first_repaint_mix(e, d, b, rows[0].sa_t, rows[0].s1m_t));
    // one 16-byte access per lane needs every tensor behind lp aligned; the decision is baked into a captured graph, so it is part of its key
    const bool aligned = aligned16(d.y_dev) && aligned4(d.mask_dev) && aligned16(noise_ps) && aligned16(d.noise_rp_dev);
    AncestralStepArgs a{};
    a.x = b.x; a.out6 = b.out6; a.mode = d.generate_mode; a.ddim = d.ddim_sample ? 1 : 0;
    a.device_noise = host ? 0 : 1; a.row = cur; a.lp = lp; a.B = B; a.HW = H * W; a.cus = e->cus; a.scalar_only = aligned ? 0 : 1;

    StepLoop L{n_rows, rows_dev, cur, sizeof(AncestralRowDev)};
    // repaint: a row that mixed the next one in left its own x in the scratch image
    L.panel_x = [&](int r) { return premix && rows[r].mix_next ? e->progress_premix : b.x; };
    L.slot_of = [](int) { return 0; };
    L.step = [&](int) -> Status {
        DPIR_TRY(denoise(e, b, &cur->st));
        ProfScope ps(&e->prof, PC_ELEM);
        return launch_ancestral_step(e->stream, a);
    };
    L.key_of = [&](int) {
        dpir_engine::GraphKey k{};
        k.task = d.task; k.B = B; k.H = H; k.W = W; k.sf = 1; k.generate_mode = d.generate_mode;
        k.kind = (aligned ? 1 : 0) | (d.ddim_sample ? 2 : 0);
        k.host_n2 = host; k.host_rp = d.noise_rp_dev != nullptr;
        k.has_labels = d.labels_host != nullptr;
        k.loop = 2;
        return k;
    };
    return run_steps(e, d, b, L, out_f32, out_u8);
}

int dpir_run_ancestral_loop(dpir_engine* e, const dpir_loop_desc* dd, const dpir_ancestral_row* rows, int n_rows, const float* noise_ps,
                            float* out_f32, uint8_t* out_u8) {
    ProgressOneShot one_shot{e};
    return run_with_hop_guard(e, [&] { return run_ancestral_loop_once(e, dd, rows, n_rows, noise_ps, out_f32, out_u8); });
}

// ------------------------------------------------------------------------------------------ gradient-mode plugs + DPS loop (8f-4)
// The batch-wide residual norm from the per-workgroup partial sums.  With a communicator of more than one rank the squared sums are
// all-reduced first: DPS_y0's update x = xt - d norm / d x has no `* norm` factor, so the GLOBAL batch norm of the reference
// (torch.linalg.norm over the whole batch, utils_model.py:392) must be used or the result would depend on the sharding.
static Status dps_norm(dpir_engine* e, const double* part, int nparts, float* normv) {
    double* ssq = nullptr;
    DPIR_TRY(e->ws.getT("dps#ssq", (size_t)2, &ssq));
    DPIR_TRY(launch_norm_fold_ssq(e->stream, part, nparts, ssq));
    if (e->comm && e->comm_world > 1) DPIR_TRY(comm_allreduce_sum_f64(e, ssq, 1));
    return launch_norm_sqrt(e->stream, ssq, normv);
}

// model_fn(..., 'pred_x_prev_and_start') = one denoiser call + p_sample / ddim_sample(eta = 0) (utils_model.py:219-243).  In gradient mode the
// forward leaves its tape and the clamp mask behind for dps_grad_through_network.
static Status p_sample_impl(dpir_engine* e, const float* x, const int* t_dev, const int* y_dev, const PSampleCoef& cf, const float* noise, float* out6,
                            float* xt, float* x0, int B, int H, int W) {
    const int oc = e->net.desc.out_channels;
    if (oc != 6) return Status{DPIR_ERR_UNSUPPORTED, "p_sample needs a learn_sigma model (out_channels == 6): the learned-range variance is read from channels 3..5"};
    unsigned char* inside = nullptr;
    DPIR_TRY(e->ws.getT("dps#inside", (size_t)B * 3 * H * W, &inside));
    DPIR_TRY(unet_forward(e, x, t_dev, y_dev, out6, B, H, W, nullptr, nullptr, true));      // every caller passes one timestep for the whole batch
    ProfScope ps(&e->prof, PC_ELEM);
    DPIR_TRY(launch_psample(e->stream, x, out6, oc, noise, cf, x0, xt, inside, B, H * W));
    e->ps_c1 = cf.c1; e->ps_c2 = cf.c2; e->ps_B = B; e->ps_H = H; e->ps_W = W; e->ps_x0 = x0; e->ps_serial = e->fwd_serial;
    return Status{};
}

// The measurement operator of the gradient modes, the one thing the two families differ in: Resizer(1 / sf) (k == nullptr; ONE residual norm for
// the whole batch, all-reduced over the communicator) or the deblurring program's reflect-padded blur Tx with one K x K PSF per image (sf 1; one
// norm PER IMAGE, no collective).  The measurement itself is a BlurResidual's y / noise / ma / mb / sa / s1m / qa / qb for both.
struct GradOp {
    int sf = 1; const float* k = nullptr; int K = 0;
    int norm_images(int B) const { return k ? B : 0; }        // the `images` of launch_grad_step / launch_neg_scale_by_norm, the floats of the norm (0: one)
    size_t measurement_count(int B, int H, int W) const { return (size_t)B * 3 * (H / sf) * (W / sf); }
};

// d || m - Resizer(x_hat) || / d x_hat, un-normalised: diff = m - Resizer(x_hat) (kept), the norm (device float), gup = Resizer^T diff.
// measurement = sa (ma y + mb) + s1m noise (qa / qb are the blur operator's).
static Status dps_residual(dpir_engine* e, const float* x_hat, const BlurResidual& meas, int sf, int B, int H, int W, float** gup_out, float** norm_out) {
    const int h = H / sf, w = W / sf;
    const size_t total = (size_t)B * 3 * H * W, small = (size_t)B * 3 * h * w;
    hipStream_t s = e->stream;
    float *down = nullptr, *diff = nullptr, *gmid = nullptr, *gup = nullptr, *normv = nullptr; double* part = nullptr;
    DPIR_TRY(e->ws.getT("dps#down", small, &down));
    DPIR_TRY(e->ws.getT("dps#diff", small, &diff));
    DPIR_TRY(e->ws.getT("dps#gmid", (size_t)B * 3 * h * W, &gmid));
    DPIR_TRY(e->ws.getT("dps#gup", total, &gup));
    DPIR_TRY(e->ws.getT("dps#part", (size_t)256, &part));
    DPIR_TRY(e->ws.getT("dps#norm", (size_t)4, &normv));
    ResizerTab th, tw;
    DPIR_TRY(e->resizer(H, sf, &th));
    DPIR_TRY(e->resizer(W, sf, &tw));
    DPIR_TRY(resize_down_impl(e, x_hat, 1.f, 0.f, down, sf, B, H, W));
    DPIR_TRY(launch_diff_norm(s, meas.y, meas.ma, meas.mb, down, diff, small, part, 256, nullptr, meas.sa, meas.s1m, meas.noise));
    DPIR_TRY(dps_norm(e, part, 256, normv));
    // Resizer^T: the forward resamples dim 2 (H) first, then dim 3 (W) -> adjoint W first, then H
    DPIR_TRY(launch_band_resample_T(s, diff, tw.w, tw.idx, tw.taps, B * 3 * h, W, w, 1, 1.f, gmid));
    DPIR_TRY(launch_band_resample_T(s, gmid, th.w, th.idx, th.taps, B * 3, H, h, W, 1.f, gup));
    *gup_out = gup; *norm_out = normv;
    return Status{};
}

static Status blur_adjoint_impl(dpir_engine* e, const float* g, const float* k, int K, float xa, float* gx, int B, int H, int W) {
    float* pad = nullptr;
    DPIR_TRY(e->ws.getT("blur#pad", (size_t)B * 3 * (H + K - 1) * (W + K - 1), &pad));
    return launch_blur_reflect_adjoint(e->stream, g, k, K, xa, pad, gx, B, H, W);
}

// difference = m - Tx(x_hat) (main_ddpir_deblur.py:307-311), one norm PER IMAGE (the program restores one image at a time, so utils_model.py:392 sees a
// batch of one), gup = Tx^T difference = 0.5 R^T C^T difference.  m = (sa (ma y + mb) + s1m noise) qa + qb.
static Status blur_residual(dpir_engine* e, const float* x_hat, const BlurResidual& meas, const float* k, int K, int B, int H, int W,
                            float** gup_out, float** norm_out) {
    const size_t total = (size_t)B * 3 * H * W;
    const int per_img = 3 * blur_tiles(H, W);
    BlurResidual r = meas;
    float *gup = nullptr, *normv = nullptr;
    DPIR_TRY(e->ws.getT("blur#diff", total, &r.diff));
    DPIR_TRY(e->ws.getT("blur#part", (size_t)B * per_img, &r.part));
    DPIR_TRY(e->ws.getT("blur#norm", (size_t)(B < 4 ? 4 : B), &normv));
    DPIR_TRY(e->ws.getT("blur#gup", total, &gup));
    DPIR_TRY(launch_blur_reflect(e->stream, x_hat, k, K, 0.5f, 0.5f, nullptr, B, H, W, &r));
    DPIR_TRY(launch_norm_fold_per_image(e->stream, r.part, per_img, B, normv));
    DPIR_TRY(blur_adjoint_impl(e, r.diff, k, K, 0.5f, gup, B, H, W));
    *gup_out = gup; *norm_out = normv;
    return Status{};
}

// gup = A^T (m - A(x_hat)), un-normalised, and || m - A(x_hat) || (one float, or one per image) for the operator A of `op`
static Status grad_residual(dpir_engine* e, const GradOp& op, const float* x_hat, const BlurResidual& meas, int B, int H, int W,
                            float** gup_out, float** norm_out) {
    if (op.k) return blur_residual(e, x_hat, meas, op.k, op.K, B, H, W, gup_out, norm_out);
    return dps_residual(e, x_hat, meas, op.sf, B, H, W, gup_out, norm_out);
}

// torch.autograd.grad(norm, x) with x_hat = x0 of the last p_sample_impl(x): the clamp mask, the direct c1 term and the network backward.
// Leaves direct / dx_net in the workspace (norm_grad = direct + dx_net).
static Status dps_grad_through_network(dpir_engine* e, const float* gup, const float* normv, float** direct_out, float** dxn_out, bool norm_per_image) {
    const int B = e->ps_B, H = e->ps_H, W = e->ps_W, oc = e->net.desc.out_channels;
    const size_t total = (size_t)B * 3 * H * W;
    float *dout6 = nullptr, *direct = nullptr, *dxn = nullptr; unsigned char* inside = nullptr;
    DPIR_TRY(e->ws.getT("dps#dout6", (size_t)B * oc * H * W, &dout6));
    DPIR_TRY(e->ws.getT("dps#direct", total, &direct));
    DPIR_TRY(e->ws.getT("dps#dxn", total, &dxn));
    DPIR_TRY(e->ws.getT("dps#inside", total, &inside));
    DPIR_TRY(launch_dps_seed(e->stream, gup, normv, inside, e->ps_c1, e->ps_c2, oc, dout6, direct, B, H * W, norm_per_image));
    DPIR_TRY(unet_backward(e, dout6, dxn));
    *direct_out = direct; *dxn_out = dxn;
    return Status{};
}

int dpir_p_sample(dpir_engine* e, const float* x_dev, int t, const dpir_psample_coef* c, const float* noise_dev, const int64_t* y_host,
                  float* xt_out_dev, float* x0_out_dev, int B, int H, int W) {
    if (!e || !x_dev || !c || !noise_dev || !xt_out_dev || !x0_out_dev || B <= 0 || H <= 0 || W <= 0) return fail(e, invalid("dpir_p_sample: bad argument"));
    (void)hipSetDevice(e->device);
    if (!e->net.loaded) return fail(e, Status{DPIR_ERR_STATE, "dpir_load_unet has not been called"});
    API_TRY(e, labels_match(e, y_host));
    range_clear(e);
    int *t_dev = nullptr, *y_dev = nullptr;
    float* out6 = nullptr;
    API_TRY(e, fill_ints(e, "api#t", t, B, &t_dev));
    API_TRY(e, upload_ints(e, "api#y", y_host, B, &y_dev));
    API_TRY(e, e->ws.getT("loop#out6", (size_t)B * e->net.desc.out_channels * H * W, &out6));
    PSampleCoef cf{c->c1, c->c2, c->pc1, c->pc2, c->min_log, c->max_log, t != 0 ? 1.0f : 0.0f, c->ddim, c->sa_prev, c->s1m_prev};
    API_TRY(e, p_sample_impl(e, x_dev, t_dev, y_dev, cf, noise_dev, out6, xt_out_dev, x0_out_dev, B, H, W));
    if (!e->fuse_h1_off && !e->grad_enabled && e->precision != 0) {
        std::vector<int64_t> yv;
        if (y_host) yv.assign(y_host, y_host + B);
        const dpir_psample_coef cc = *c;
        if (x_dev != xt_out_dev && x_dev != x0_out_dev)
            e->arm_replay([=]() { return dpir_p_sample(e, x_dev, t, &cc, noise_dev, yv.empty() ? nullptr : yv.data(), xt_out_dev, x0_out_dev, B, H, W); });
        else { ++e->fwd_since_sync; e->replay_last = nullptr; }
    }
    return DPIR_OK;
}

int dpir_eps_from_xstart(dpir_engine* e, const float* x_dev, const float* x0_dev, float sqrt_ac, float sqrt_1m_ac, int score, float* out_dev, size_t numel) {
    if (!e || !x_dev || !x0_dev || !out_dev) return fail(e, invalid("dpir_eps_from_xstart: null argument"));
    (void)hipSetDevice(e->device);
    ProfScope ps(&e->prof, PC_ELEM);
    API_TRY(e, launch_eps_from_xstart(e->stream, x_dev, x0_dev, sqrt_ac, sqrt_1m_ac, score, out_dev, numel));
    return DPIR_OK;
}

// utils_model.grad_and_value over the operator of `op`, the body of dpir_grad_and_value and dpir_grad_and_value_blur (their arguments are checked):
// norm_grad_out = d norm / d x, norm_out (may be null) = the norm, one float or one per image.
static int grad_and_value_impl(dpir_engine* e, int through_network, const float* x_hat_dev, const float* measurement_dev, const GradOp& op,
                               float* norm_grad_out_dev, float* norm_out_dev, int B, int H, int W) {
    (void)hipSetDevice(e->device);
    const size_t total = (size_t)B * 3 * H * W;
    const int images = op.norm_images(B);
    if (through_network) {
        if (!e->grad_enabled) return fail(e, Status{DPIR_ERR_STATE, "grad_and_value through the denoiser needs gradient mode: dpir_enable_grad before dpir_load_unet"});
        if (!e->tape.valid || e->tape.serial != e->ps_serial || e->ps_serial != e->fwd_serial || e->ps_x0 != x_hat_dev || e->ps_B != B || e->ps_H != H || e->ps_W != W)
            return fail(e, Status{DPIR_ERR_STATE, "grad_and_value(x, x_hat): x_hat must be the pred_xstart output of the LAST dpir_p_sample call on this engine "
                                                  "(the tape of that forward is what the gradient runs through)"});
    }
    ProfScope ps(&e->prof, PC_ELEM);
    float *gup = nullptr, *normv = nullptr;
    BlurResidual meas; meas.y = measurement_dev;
    API_TRY(e, grad_residual(e, op, x_hat_dev, meas, B, H, W, &gup, &normv));
    if (through_network) {
        float *direct = nullptr, *dxn = nullptr;
        API_TRY(e, dps_grad_through_network(e, gup, normv, &direct, &dxn, images != 0));
        API_TRY(e, launch_dps_update(e->stream, nullptr, direct, dxn, 0.f, nullptr, norm_grad_out_dev, total));
    } else {
        // norm_grad = -gup / norm: grad_step with src = 0, lam * nv / rho * tail = 1  ->  dst = 0 - ng  ... evaluated as a plain scale instead
        API_TRY(e, launch_neg_scale_by_norm(e->stream, gup, normv, norm_grad_out_dev, total, images));
    }
    if (norm_out_dev) API_HIP(e, hipMemcpyAsync(norm_out_dev, normv, sizeof(float) * (images ? images : 1), hipMemcpyDeviceToDevice, e->stream));
    return DPIR_OK;
}

int dpir_grad_and_value(dpir_engine* e, int through_network, const float* x_hat_dev, const float* measurement_dev, int sf, float* norm_grad_out_dev,
                        float* norm_out_dev, int B, int H, int W) {
    if (!e || !x_hat_dev || !measurement_dev || !norm_grad_out_dev) return fail(e, invalid("dpir_grad_and_value: null argument"));
    API_TRY(e, check_shape("dpir_grad_and_value", B, H, W, sf));
    GradOp op; op.sf = sf;
    return grad_and_value_impl(e, through_network, x_hat_dev, measurement_dev, op, norm_grad_out_dev, norm_out_dev, B, H, W);
}

// What both whole-loop entries of the gradient modes refuse ahead of their own task / shape checks (and behind "no model")
static Status grad_loop_ready(dpir_engine* e, int variant) {
    if (variant == 0 && !e->grad_enabled) return Status{DPIR_ERR_STATE, "DPS_y0 needs gradient mode: dpir_enable_grad before dpir_load_unet"};
    return Status{};
}

// The loop of the gradient modes over the operator of `op`: the body of dpir_run_dps_loop (main_ddpir.py:291-470) and dpir_run_deblur_grad_loop
// (main_ddpir_deblur.py:228-360), which pass what they refuse about the task, the shape and the variants they admit as `own`.  The operator decides
// the image the initial x is noised from (bicubic up-sampling of y | y), the measurement ((2y - 1) and sa_t (2y - 1) + s1m_t n | y and that / 2 + 0.5),
// the extent of the y_t draw and whether the norm is the batch's or each image's.  Eager launches, no step graph: only the head, the
// initialisation and the tail are the other loops'.
static int run_grad_loop(dpir_engine* e, const char* entry, const Status& own, const dpir_loop_desc& d, const dpir_step* steps, const dpir_dps_coef* coefs,
                         int n_steps, int variant, float lambda_, const float* noise_ps_dev, const float* noise_yt_dev, float step_scale, const GradOp& op,
                         float* out_f32, uint8_t* out_u8) {
    bool with_n1 = false;
    LoopCall c{entry, n_steps, "step", std::vector<char>(n_steps)};
    for (int i = 0; i < n_steps; ++i) {
        c.last[i] = steps[i].last != 0;
        if (variant == 2 && !steps[i].last && steps[i].es != 0.f) with_n1 = true;
    }
    c.modes = nullptr; c.x0 = true; c.n1 = with_n1; c.init = !op.k;
    c.own = own;
    if (own.ok() && with_n1 && d.noise_n2_dev && !d.noise_n1_dev) c.own = invalid(std::string(entry) + ": eta != 0 with host noise needs noise_n1_dev");
    LoopBufs b{};
    if (int rc = loop_prologue(e, c, d, &b)) return rc;
    const int B = d.B, H = d.H, W = d.W, oc = e->net.desc.out_channels, images = op.norm_images(B);
    const size_t total = (size_t)B * 3 * H * W, small = op.measurement_count(B, H, W);
    hipStream_t s = e->stream;
    float* xprev = nullptr;
    API_TRY(e, e->ws.getT("dps#xprev", total, &xprev));
    // init: the Resizer noises the bicubic up-sampling of y to t_start (main_ddpir.py:293-315); the deblurring program noises y itself from its own
    // level t_y up to t_start (main_ddpir_deblur.py:228-231): no mask, and no spectra although its task is deblur
    API_TRY(e, loop_init(e, d, b, op.k ? 0 : op.sf, nullptr, nullptr));
    for (int i = 0; i < n_steps; ++i) {
        API_TRY(e, progress_emit(e, i - 1, b.x, d));     // the panel of step i - 1: x after its update
        const dpir_step& st = steps[i];
        if (st.last && d.skip_dead_final_eval) continue;
        std::vector<int64_t> tv(B, st.t);
        int* t_dev = nullptr;
        API_TRY(e, upload_ints(e, "loop#tt", tv.data(), B, &t_dev));
        if (st.last) {                                            // the final denoiser call is dead (main_ddpir.py:384, 470; main_ddpir_deblur.py:284, 339, 360)
            API_TRY(e, unet_forward(e, b.x, t_dev, b.y_dev, b.out6, B, H, W));
            continue;
        }
        float *gup = nullptr, *normv = nullptr;
        BlurResidual meas; meas.y = d.y_dev;                      // Tx is measured against y in [0, 1] (main_ddpir_deblur.py:312, 324) ...
        if (!op.k) { meas.ma = 2.f; meas.mb = -1.f; }             // ... the Resizer against 2y - 1 (utils_model.py:391-392)
        if (variant == 2) {
            // first-order data step (main_ddpir_deblur.py:305-314) in place of the closed-form prox, then the usual re-noise (:339-347)
            API_TRY(e, unet_forward(e, b.x, t_dev, b.y_dev, b.out6, B, H, W, nullptr, nullptr, true));
            ProfScope ps(&e->prof, PC_ELEM);
            API_TRY(e, launch_xstart(s, b.x, b.out6, oc, st.c1, st.c2, b.x0, B, H * W));
            API_TRY(e, grad_residual(e, op, b.x0, meas, B, H, W, &gup, &normv));
            API_TRY(e, launch_grad_step(s, b.x0, gup, normv, 1.f, st.tau, 1.f, b.x0, total, nullptr, images));
            const float *n1 = nullptr, *n2 = nullptr;
            if (st.es != 0.f) {
                if (d.noise_n1_dev) n1 = d.noise_n1_dev + (size_t)i * total;
                else { API_TRY(e, launch_randn(s, b.n1, d.seed, (uint64_t)4 * i + 1, d.image_offset, B, (size_t)3 * H * W)); n1 = b.n1; }
            }
            if (d.noise_n2_dev) n2 = d.noise_n2_dev + (size_t)i * total;
            else { API_TRY(e, launch_randn(s, b.n2, d.seed, (uint64_t)4 * i + 2, d.image_offset, B, (size_t)3 * H * W)); n2 = b.n2; }
            API_TRY(e, launch_renoise(s, b.x, b.x0, coef_of(st), n1, n2, total));
            continue;
        }
        const float* nz = noise_ps_dev ? noise_ps_dev + (size_t)i * total : nullptr;
        if (!nz) { ProfScope ps(&e->prof, PC_ELEM); API_TRY(e, launch_randn(s, b.n2, d.seed, (uint64_t)4 * (i + 1), d.image_offset, B, (size_t)3 * H * W)); nz = b.n2; }
        PSampleCoef cf{st.c1, st.c2, coefs[i].pc1, coefs[i].pc2, coefs[i].min_log, coefs[i].max_log, st.t != 0 ? 1.0f : 0.0f,
                       d.ddim_sample, coefs[i].sa_prev, coefs[i].s1m_prev};
        API_TRY(e, p_sample_impl(e, b.x, t_dev, b.y_dev, cf, nz, b.out6, xprev, b.x0, B, H, W));
        ProfScope ps(&e->prof, PC_ELEM);
        if (variant == 1) {
            // DPS_yt (main_ddpir.py:439-445, main_ddpir_deblur.py:329-336): y_t = sa_t (2y - 1) + s1m_t n, which Tx measures as y_t / 2 + 0.5; the
            // residual is taken at xt = p_sample's sample and differentiated w.r.t. xt itself -- no backward through the network.  The norm is
            // multiplied back in (:444); the Resizer's is still the whole batch's (all-reduced in dps_norm), so no bit depends on the sharding
            const float* ny = noise_yt_dev ? noise_yt_dev + (size_t)i * small : nullptr;
            if (!ny) {
                float* nyb = nullptr;
                API_TRY(e, e->ws.getT("dps#ny", small, &nyb));
                API_TRY(e, launch_randn(s, nyb, d.seed, (uint64_t)4 * (i + 1) + 1, d.image_offset, B, small / B));
                ny = nyb;
            }
            meas.ma = 2.f; meas.mb = -1.f; meas.sa = st.sa_t; meas.s1m = st.s1m_t; meas.noise = ny;
            if (op.k) meas.qa = meas.qb = 0.5f;
            API_TRY(e, grad_residual(e, op, xprev, meas, B, H, W, &gup, &normv));
            API_TRY(e, launch_grad_step(s, xprev, gup, normv, lambda_, st.tau, 0.35f, b.x, total, nullptr, images));
            continue;
        }
        // DPS_y0 (main_ddpir.py:434-438, main_ddpir_deblur.py:323-327): x = xt - step_scale d || m - A(x0) || / d x, through the clamp and the denoiser
        float *direct = nullptr, *dxn = nullptr;
        API_TRY(e, grad_residual(e, op, b.x0, meas, B, H, W, &gup, &normv));
        API_TRY(e, dps_grad_through_network(e, gup, normv, &direct, &dxn, images != 0));
        API_TRY(e, launch_dps_update(s, xprev, direct, dxn, step_scale, b.x, nullptr, total));
    }
    return loop_finish(e, d, b, n_steps, b.x, out_f32, out_u8);
}

int dpir_run_dps_loop(dpir_engine* e, const dpir_loop_desc* dd, const dpir_step* steps, const dpir_dps_coef* coefs, int n_steps,
                      int variant, float lambda_, const float* noise_ps_dev, const float* noise_yt_dev, float step_scale, float* out_f32,
                      uint8_t* out_u8) {
    ProgressOneShot one_shot{e};
    if (!e || !dd || !steps || !coefs || n_steps <= 0) return fail(e, invalid("dpir_run_dps_loop: null argument"));
    if (variant != 0 && variant != 1) return fail(e, invalid("dpir_run_dps_loop: variant must be 0 (DPS_y0) or 1 (DPS_yt)"));
    const dpir_loop_desc& d = *dd;
    const Status own = [&]() -> Status {
        DPIR_TRY(grad_loop_ready(e, variant));
        if (d.task != DPIR_TASK_SR_BLUR && d.task != DPIR_TASK_SR_CUBIC)
            return Status{DPIR_ERR_UNSUPPORTED, "DPS_y0 is implemented for the super-resolution tasks (the reference's deblurring operator raises at "
                                                "main_ddpir.py:302 and its inpainting branch never defines xt)"};
        if (d.B <= 0 || d.H <= 0 || d.W <= 0 || d.sf < 1 || d.H % d.sf || d.W % d.sf || !d.y_dev) return invalid("dpir_run_dps_loop: bad shape");
        return Status{};
    }();
    GradOp op; op.sf = d.sf;
    return run_grad_loop(e, "dpir_run_dps_loop", own, d, steps, coefs, n_steps, variant, lambda_, noise_ps_dev, noise_yt_dev, step_scale, op, out_f32, out_u8);
}

// ------------------------------------------------------------------------------------------ deblurring program: blur operator + gradient modes
int dpir_blur_reflect(dpir_engine* e, const float* x_dev, const float* k_dev, int kh, int kw, float xa, float xb, float* out_dev, int B, int H, int W) {
    if (!e || !x_dev || !k_dev || !out_dev) return fail(e, invalid("dpir_blur_reflect: null argument"));
    API_TRY(e, blur_check("dpir_blur_reflect", kh, kw, B, H, W));
    (void)hipSetDevice(e->device);
    ProfScope ps(&e->prof, PC_ELEM);
    API_TRY(e, launch_blur_reflect(e->stream, x_dev, k_dev, kh, xa, xb, out_dev, B, H, W));
    return DPIR_OK;
}

int dpir_blur_reflect_adjoint(dpir_engine* e, const float* g_dev, const float* k_dev, int kh, int kw, float xa, float* gx_dev, int B, int H, int W) {
    if (!e || !g_dev || !k_dev || !gx_dev) return fail(e, invalid("dpir_blur_reflect_adjoint: null argument"));
    API_TRY(e, blur_check("dpir_blur_reflect_adjoint", kh, kw, B, H, W));
    (void)hipSetDevice(e->device);
    ProfScope ps(&e->prof, PC_ELEM);
    API_TRY(e, blur_adjoint_impl(e, g_dev, k_dev, kh, xa, gx_dev, B, H, W));
    return DPIR_OK;
}

int dpir_grad_and_value_blur(dpir_engine* e, int through_network, const float* x_hat_dev, const float* measurement_dev, const float* k_dev, int kh, int kw,
                             float* norm_grad_out_dev, float* norm_out_dev, int B, int H, int W) {
    if (!e || !x_hat_dev || !measurement_dev || !k_dev || !norm_grad_out_dev) return fail(e, invalid("dpir_grad_and_value_blur: null argument"));
    API_TRY(e, blur_check("dpir_grad_and_value_blur", kh, kw, B, H, W));
    GradOp op; op.k = k_dev; op.K = kh;
    return grad_and_value_impl(e, through_network, x_hat_dev, measurement_dev, op, norm_grad_out_dev, norm_out_dev, B, H, W);
}

int dpir_run_deblur_grad_loop(dpir_engine* e, const dpir_loop_desc* dd, const dpir_step* steps, const dpir_dps_coef* coefs, int n_steps, int variant,
                              float lambda_, const float* noise_ps_dev, const float* noise_yt_dev, float* out_f32, uint8_t* out_u8) {
    ProgressOneShot one_shot{e};
    if (!e || !dd || !steps || n_steps <= 0) return fail(e, invalid("dpir_run_deblur_grad_loop: null argument"));
    if (variant < 0 || variant > 2) return fail(e, invalid("dpir_run_deblur_grad_loop: variant must be 0 (DPS_y0), 1 (DPS_yt) or 2 (first-order data step)"));
    if (variant != 2 && !coefs) return fail(e, invalid("dpir_run_deblur_grad_loop: the DPS variants need the p_sample coefficients"));
    const dpir_loop_desc& d = *dd;
    const Status own = [&]() -> Status {
        DPIR_TRY(grad_loop_ready(e, variant));
        if (d.task != DPIR_TASK_DEBLUR || d.sf != 1) return invalid("dpir_run_deblur_grad_loop: the deblurring program runs task deblur (sf 1) only");
        if (!d.y_dev || !d.k_dev) return invalid("dpir_run_deblur_grad_loop: y and the PSF are required");
        return blur_check("dpir_run_deblur_grad_loop", d.kh, d.kw, d.B, d.H, d.W);
    }();
    GradOp op; op.k = d.k_dev; op.K = d.kh;
    // the program's DPS_y0 update is a unit step (main_ddpir_deblur.py:326)
    return run_grad_loop(e, "dpir_run_deblur_grad_loop", own, d, steps, coefs, n_steps, variant, lambda_, noise_ps_dev, noise_yt_dev, 1.f, op, out_f32, out_u8);
}

// ------------------------------------------------------------------------------------------ profiling
int dpir_graph_cache_size(dpir_engine* e) { return e ? (int)e->graphs.size() : 0; }
int dpir_prof_enable(dpir_engine* e, int on) {
    if (!e) return DPIR_ERR_INVALID;
    e->prof.collect();
    e->prof.on = on != 0;
    return DPIR_OK;
}
int dpir_prof_reset(dpir_engine* e) {
    if (!e) return DPIR_ERR_INVALID;
    e->prof.reset();
    return DPIR_OK;
}
int dpir_prof_read(dpir_engine* e, double* ms_out, int64_t* count_out) {
    if (!e || !ms_out || !count_out) return DPIR_ERR_INVALID;
    e->prof.collect();
    for (int i = 0; i < DPIR_PROF_CLASSES; ++i) { ms_out[i] = e->prof.ms[i]; count_out[i] = e->prof.cnt[i]; }
    return DPIR_OK;
}

}  // extern "C"
