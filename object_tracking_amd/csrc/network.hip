// network.hip -- context, weight loading and layer sequencing behind the C ABI
// (include/mi355_dt.h).  Graph topology follows the reference:
//   detector  models_detection/KerasYOLO.py:277-405 (weight order :244-274)
//   tracker   models_tracking/MultiObjDetTracker.py:160-189
//   tiny      models_tracking/TinyTracker.py:25-41
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdlib>
#include <cstring>
#include <thread>

#include "dt_internal.h"

static const float BN_EPS = 1e-3f;   // Keras BatchNormalization default (no epsilon= passed)
static const float LEAKY = 0.1f;     // LeakyReLU(alpha=0.1)
static char g_static_err[512] = "";

// (idx, k, cin, cout, pool_after) -- main trunk, KerasYOLO.py:279-384
static const int TRUNK[20][5] = {
    {1, 3, 3, 32, 1},      {2, 3, 32, 64, 1},     {3, 3, 64, 128, 0},    {4, 1, 128, 64, 0},
    {5, 3, 64, 128, 1},    {6, 3, 128, 256, 0},   {7, 1, 256, 128, 0},   {8, 3, 128, 256, 1},
    {9, 3, 256, 512, 0},   {10, 1, 512, 256, 0},  {11, 3, 256, 512, 0},  {12, 1, 512, 256, 0},
    {13, 3, 256, 512, 1},  {14, 3, 512, 1024, 0}, {15, 1, 1024, 512, 0}, {16, 3, 512, 1024, 0},
    {17, 1, 1024, 512, 0}, {18, 3, 512, 1024, 0}, {19, 3, 1024, 1024, 0}, {20, 3, 1024, 1024, 0}};

static inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

int dt_fail(dt_ctx *ctx, int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (ctx) ctx->err = buf;
    else snprintf(g_static_err, sizeof(g_static_err), "%s", buf);
    return code;
}

static void graphs_clear(dt_ctx *ctx)
{
    if (ctx->graphs.empty() && ctx->graph_seen.empty()) return;
    (void)hipStreamSynchronize(ctx->stream);      // replays run on the caller's stream
    for (auto &kv : ctx->graphs) (void)hipGraphExecDestroy(kv.second);
    ctx->graphs.clear();
    ctx->graph_seen.clear();
    ctx->graph_tags.clear();
}

// the graphs whose key ends in `suffix` only (a table of their launches' pointers is about to be replaced).  The CALLER has synchronised
// ctx->stream: replays run there
static void graphs_drop(dt_ctx *ctx, const char *suffix)
{
    const std::string suf(suffix);
    const auto ends = [&](const std::string &k) { return k.size() >= suf.size() && k.compare(k.size() - suf.size(), suf.size(), suf) == 0; };
    for (auto it = ctx->graphs.begin(); it != ctx->graphs.end();) {
        if (!ends(it->first)) { ++it; continue; }
        (void)hipGraphExecDestroy(it->second);
        it = ctx->graphs.erase(it);
    }
    for (auto it = ctx->graph_seen.begin(); it != ctx->graph_seen.end();) it = ends(it->first) ? ctx->graph_seen.erase(it) : std::next(it);
    for (auto it = ctx->graph_tags.begin(); it != ctx->graph_tags.end();) it = ends(it->first) ? ctx->graph_tags.erase(it) : std::next(it);
}

// Runs `body` (a sequence of launches on ctx->stream that touches library-owned buffers only), as a replayed
// hipGraph when graphs are on: first sighting of `key` runs plainly (allocates workspaces, one-time kernel
// attribute calls), the second captures on the internal stream and instantiates, later ones replay.
//   in_tensor: the tensor the sequence reads from outside (or null).  A replay runs no host code, so what the host knows about a tensor's
//   max |x| when the graph is captured must hold at every replay: the tag of `in_tensor` -- "its producer, which ran just before in this
//   call, published into slot s" -- is kept and becomes part of the key (another precondition, another graph); every other tag is dropped,
//   i.e. the sequence measures whatever else it reads itself.  What the sequence leaves behind is re-applied on replay.
static int graphed(dt_ctx *ctx, const std::string &key_in, const std::function<int()> &body, const float *in_tensor = nullptr)
{
    if (!ctx->graph_on || ctx->prof || ctx->capturing) return body();
    hipStream_t user = ctx->stream;
    std::string key = key_in;
    {
        std::vector<dt_ctx::AmaxTag> keep;
        for (const auto &t : ctx->amax_tag)
            if (in_tensor && t.lo == in_tensor) { keep.push_back(t); key += ":am" + std::to_string(t.slot) + "c" + std::to_string(t.cols); }
        ctx->amax_tag.swap(keep);
    }
    auto it = ctx->graphs.find(key);
    if (it == ctx->graphs.end()) {
        int &seen = ctx->graph_seen[key];
        if (seen < 0 || seen++ == 0) { const int rc0 = body(); ctx->graph_tags[key] = ctx->amax_tag; return rc0; }
        hipGraph_t g = nullptr;
        if (hipStreamBeginCapture(ctx->gstream, hipStreamCaptureModeThreadLocal) != hipSuccess) { seen = -1; return body(); }
        ctx->capturing = true; ctx->stream = ctx->gstream;
        const int rc = body();
        ctx->graph_tags[key] = ctx->amax_tag;
        ctx->stream = user; ctx->capturing = false;
        const hipError_t e = hipStreamEndCapture(ctx->gstream, &g);
        hipGraphExec_t ex = nullptr;
        if (rc != DT_OK || e != hipSuccess || !g || hipGraphInstantiate(&ex, g, nullptr, nullptr, 0) != hipSuccess) {
            if (g) (void)hipGraphDestroy(g);
            (void)hipGetLastError();
            ctx->graph_seen[key] = -1;      // do not try again for this shape
            return rc != DT_OK ? rc : body();
        }
        (void)hipGraphDestroy(g);
        ++ctx->graph_captures;
        it = ctx->graphs.emplace(key, ex).first;
    }
    // the instantiated graph is launched on the CALLER's stream (only the capture needs the internal one): stream order is the
    // synchronisation -- no event pair per replay (round 3 replayed on the internal stream between two events and was 0.06 ms
    // SLOWER than plain launches at batch 8)
    HIP_TRY(ctx, hipGraphLaunch(it->second, user));
    ctx->amax_tag = ctx->graph_tags[key];
    ++ctx->graph_replays;
    return DT_OK;
}

extern "C" int dt_graph_enable(dt_ctx *ctx, int on)
{
    if (!ctx) return DT_ERR_ARG;
    if (on && !ctx->gstream) HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->gstream, hipStreamNonBlocking));
    if (!on) graphs_clear(ctx);
    ctx->graph_on = on != 0;
    return DT_OK;
}

float *ws_get(dt_ctx *ctx, const char *name, size_t bytes, bool zero_on_grow)
{
    DevBuf &b = ctx->ws[name];
    if (b.bytes < bytes) {
        if (ctx->capturing) {   // cannot allocate inside a stream capture (graphed() runs every shape once uncaptured first)
            dt_fail(ctx, DT_ERR_STATE, "workspace %s would grow during graph capture", name);
            return nullptr;
        }
        graphs_clear(ctx);      // captured kernels hold the old pointer
        if (b.p) {
            (void)hipStreamSynchronize(ctx->stream);
            (void)hipFree(b.p);
            b.p = nullptr;
            b.bytes = 0;
        }
        if (hipMalloc(&b.p, bytes) != hipSuccess) {
            b.p = nullptr;
            dt_fail(ctx, DT_ERR_DEVICE, "hipMalloc(%zu) failed for workspace %s", bytes, name);
            return nullptr;
        }
        b.bytes = bytes;
        b.layout = 0;
        if (zero_on_grow) (void)hipMemsetAsync(b.p, 0, bytes, ctx->stream);
    }
    return static_cast<float *>(b.p);
}

// A workspace whose rows carry pad columns that no kernel writes and the GEMM behind it reads (trk_z, tiny_x): zero when it is allocated, and zeroed once
// more when a call arrives with another row layout than the one before it -- after dt_tracker_load / dt_tiny_load for another class count or D the new
// rows' pads lie on bytes that held activations (0 * NaN is NaN, and the fp16 form's max |x| is taken over the padded width).  Calls that keep the
// layout -- the steady state -- add no launch: the pads sit at the same offsets whatever the number of rows.
float *ws_get_padded(dt_ctx *ctx, const char *name, size_t bytes, int width, int used)
{
    float *p = ws_get(ctx, name, bytes, /*zero_on_grow=*/true);
    if (!p) return nullptr;
    DevBuf &b = ctx->ws[name];
    const long long layout = ((long long)width << 32) | (unsigned)used;
    if (b.layout != layout) {
        if (b.layout != 0 && width > used) {      // (0: allocated and zeroed just now; rows without pad columns have nothing to keep zero)
            if (ctx->capturing) {   // a memset recorded into a graph would run at every replay (graphed() runs every shape once uncaptured first: not reached today)
                dt_fail(ctx, DT_ERR_STATE, "workspace %s would be zeroed during graph capture", name);
                return nullptr;
            }
            if (hipMemsetAsync(b.p, 0, b.bytes, ctx->stream) != hipSuccess) {
                dt_fail(ctx, DT_ERR_DEVICE, "hipMemsetAsync failed for workspace %s", name);
                return nullptr;
            }
        }
        b.layout = layout;
    }
    return p;
}

ProfScope::ProfScope(dt_ctx *c, const char *name, double flops, double bytes, const char *tag)
    : ctx(c), on(c->prof && !c->capturing)
{
    if (!on) return;
    ev.name = name;
    if (tag) ev.tag = std::string(name) + ":" + tag;
    (void)hipEventCreate(&ev.a);
    (void)hipEventCreate(&ev.b);
    ProfEntry &e = ctx->prof_tab[name];
    e.launches += 1;
    e.flops += flops;
    e.bytes += bytes;
    if (tag) {
        ProfEntry &t = ctx->prof_tab[ev.tag];
        t.launches += 1;
        t.flops += flops;
        t.bytes += bytes;
    }
    (void)hipEventRecord(ev.a, ctx->stream);
}
ProfScope::~ProfScope()
{
    if (!on) return;
    (void)hipEventRecord(ev.b, ctx->stream);
    ctx->pending.push_back(ev);
}
// a counter without a time: which variant a launch took (the configuration parity tests assert these); the name is only built while profiling
static void prof_count(dt_ctx *ctx, const char *fmt, ...)
{
    if (!ctx->prof || ctx->capturing) return;
    char name[48];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(name, sizeof(name), fmt, ap);
    va_end(ap);
    ctx->prof_tab[name].launches += 1;
}
// what a launcher's non-zero return code means: 2 = it refused the arguments, anything else = the device did
static int launch_code(int rc) { return rc == 2 ? DT_ERR_ARG : DT_ERR_DEVICE; }

// ---- max-|x| slots of the fp16 form (dt_internal.h: dt_ctx::amax) ------------------------------------------------------------------
#define DT_AMAX_SLOTS 128
enum { AMAX_ONE = 0, AMAX_IN = 32, AMAX_TRK = 56, AMAX_TEST = 57, AMAX_PACK = 64 };
static unsigned *amax_slot(dt_ctx *ctx, int slot) { return ctx->amax ? ctx->amax.get() + (size_t)slot * DT_AMAX_WORDS : nullptr; }
// every API entry that runs layers starts here: what a previous call knew about a tensor's maximum says nothing about the bytes behind the pointer now,
// and a call of fewer than Policy::h2_minframes frames takes no fp16 form (frames = 0: a layer-level test entry, never small)
static void call_begin(dt_ctx *ctx, int frames)
{
    ctx->amax_tag.clear();
    ctx->h2_small = frames > 0 && frames < ctx->pol.h2_minframes;
}
// the slot that holds max |x| of the rows x cols tensor at x: the one its producer filled (tagged), else measured here into `slot`
// a layer is about to write `floats` floats from `lo` on: what was known about tensors in that range is void
static void amax_forget(dt_ctx *ctx, const float *lo, long long floats)
{
    if (!lo || ctx->amax_tag.empty()) return;
    const float *hi = lo + floats;
    auto &v = ctx->amax_tag;
    for (size_t i = v.size(); i-- > 0;)
        if (v[i].lo < hi && lo < v[i].hi) v.erase(v.begin() + (long)i);
}
static void amax_note(dt_ctx *ctx, const float *lo, long long floats, int cols, int slot)
{
    amax_forget(ctx, lo, floats);
    ctx->amax_tag.push_back(dt_ctx::AmaxTag{lo, lo + floats, cols, slot});
}
// the producers' slots of one detector forward start from zero (the epilogues only ever raise them)
static int amax_begin(dt_ctx *ctx)
{
    if (!ctx->amax) return DT_OK;
    HIP_TRY(ctx, hipMemsetAsync(amax_slot(ctx, 1), 0, (size_t)(AMAX_IN - 1) * DT_AMAX_WORDS * sizeof(unsigned), ctx->stream));
    return DT_OK;
}
// slot a layer's epilogue fills with the max |x| of what it writes: conv_1 .. conv_23 only (the test entry points run "layer 0")
static int amax_out_slot(const ConvLayer &L) { return L.idx >= 1 && L.idx <= 23 ? L.idx : 0; }
// slot a layer's input is measured into where no producer published it
static int amax_in_slot(const ConvLayer &L) { return L.idx >= 1 && L.idx <= 23 ? AMAX_IN + L.idx : AMAX_TEST; }
static const unsigned *ensure_amax(dt_ctx *ctx, const float *x, long long rows, int cols, long long ld, int slot)
{
    if (!ctx->pol.amax_measure)      // (DT_AMAX_MEASURE: measure what a producer published too, so that the two words can be compared)
        for (const auto &t : ctx->amax_tag)
            if (t.lo == x && t.hi == x + rows * ld && t.cols == cols) return amax_slot(ctx, t.slot);
    unsigned *s = amax_slot(ctx, slot);
    if (!s) { dt_fail(ctx, DT_ERR_STATE, "max-|x| slots not allocated"); return nullptr; }
    char tag[16];      // whose input this is: absmax:conv_i / absmax:trk / absmax:test
    if (slot > AMAX_IN && slot < AMAX_TRK) snprintf(tag, sizeof(tag), "conv_%d", slot - AMAX_IN);
    else snprintf(tag, sizeof(tag), "%s", slot == AMAX_TRK ? "trk" : "test");
    ProfScope ps(ctx, "absmax", 0.0, 4.0 * (double)rows * cols, tag);
    if (launch_absmax(ctx->stream, x, rows, cols, ld, 1, 0, s)) { dt_fail(ctx, DT_ERR_DEVICE, "absmax launch failed"); return nullptr; }
    for (const auto &t : ctx->amax_tag)      // (a slot names ONE tensor)
        if (t.slot == slot) { amax_forget(ctx, t.lo, t.hi - t.lo); break; }
    amax_note(ctx, x, rows * ld, cols, slot);
    return s;
}
// does this launch take the fp16 form of the split GEMM?  (DT_PIN keeps the bf16 form: see Policy::s3_h2)
static bool h2_wanted(const dt_ctx *ctx) { return ctx->pol.s3 != 0 && ctx->pol.s3_h2 != 0 && !ctx->pol.pin && !ctx->h2_small; }

// host array -> a fresh device allocation; `dst` takes it (and releases what it held) only when the copy succeeded
template <class T> static int upload(dt_ctx *ctx, DevMem<T> &dst, const std::vector<T> &h)
{
    DevMem<T> d;
    HIP_TRY(ctx, d.alloc(h.size()));
    HIP_TRY(ctx, hipMemcpy(d.get(), h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
    dst = std::move(d);
    return DT_OK;
}

// ---- kernel-selection policy (dt_internal.h: Policy) ------------------------------------------------------------------------------
// the integer knobs and their environment variables; DT_WINO_WS_GB (a double) and the two derived fp16-form row thresholds are read after the loop
static const struct { const char *name; int Policy::*field; } k_knobs[] = {
    {"DT_WINO", &Policy::wino}, {"DT_WINO_TILE", &Policy::wino_tile}, {"DT_WINO_MINT", &Policy::wino_mint},
    {"DT_WINO_MOSAIC", &Policy::mosaic}, {"DT_WINO_FUSED4", &Policy::fused4}, {"DT_TRK_MERGE", &Policy::trk_merge},
    {"DT_PIN", &Policy::pin}, {"DT_C3H2", &Policy::c3h2}, {"DT_C3FUSE", &Policy::c3fuse}, {"DT_CONV_CFG", &Policy::conv_cfg},
    {"DT_S3", &Policy::s3}, {"DT_S3_CONV1", &Policy::s3_conv1}, {"DT_S3_MINROWS", &Policy::s3_minrows}, {"DT_S3_H2", &Policy::s3_h2},
    {"DT_H2_MINFRAMES", &Policy::h2_minframes}, {"DT_S3_HALF", &Policy::s3_half}, {"DT_S3_REC_MINROWS", &Policy::s3_rec_minrows},
    {"DT_S3_1X1", &Policy::s3_1x1}, {"DT_S3_1X1_MINK", &Policy::s3_1x1_mink}, {"DT_S3_1X1_MINROWS", &Policy::s3_1x1_minrows},
    {"DT_AMAX_MEASURE", &Policy::amax_measure},
};

static void policy_from_env(Policy &p)
{
    const Policy d;
    for (const auto &k : k_knobs) {
        const char *e = getenv(k.name);
        p.*k.field = e ? atoi(e) : d.*k.field;
    }
    { const char *e = getenv("DT_WINO_WS_GB"); p.wino_ws_gb = e ? atof(e) : d.wino_ws_gb; }
    p.s3_minrows_h2 = getenv("DT_S3_MINROWS") ? p.s3_minrows : d.s3_minrows_h2;
    p.s3_rec_minrows_h2 = getenv("DT_S3_REC_MINROWS") ? p.s3_rec_minrows : d.s3_rec_minrows_h2;
}

static bool policy_equal(const Policy &a, const Policy &b)
{
    for (const auto &k : k_knobs)
        if (a.*k.field != b.*k.field) return false;
    return a.wino_ws_gb == b.wino_ws_gb && a.s3_minrows_h2 == b.s3_minrows_h2 && a.s3_rec_minrows_h2 == b.s3_rec_minrows_h2;
}

// The one writer of ctx->pol: the environment, then the context's pin override (dt_policy_set), then what DT_PIN implies.  Captured
// graphs hold the launches of the policy they were captured under: any change drops them.
static void policy_refresh(dt_ctx *ctx)
{
    Policy p;
    policy_from_env(p);
    if (ctx->pin_override >= 0) p.pin = ctx->pin_override;
    if (p.pin) {      // every choice below otherwise looks at the number of frames / rows / tiles of the launch (no split-K either: run_conv)
        p.wino = 2; p.mosaic = 1; p.fused4 = 2; p.s3_half = -1;
        if (p.s3) p.s3 = 2;
        p.trk_merge = 0;      // ONE form of the input projection, whichever entry point carries the frame (the merged weights are a different rounding of the
                              // same network, and dt_track_recurrent on a caller's z rows cannot take them)
        // (the fp16 form of the split GEMM is off under DT_PIN as well: h2_wanted)
    }
    if (!policy_equal(p, ctx->pol)) graphs_clear(ctx);
    ctx->pol = p;
}

// ---------------------------------------------------------------------------
extern "C" int dt_abi_version(void) { return 108; }   // 1.08: + dt_amax_read, the four dt_*stream* entries (1.07: + dt_gemm_split, dt_policy_set)

// the host's view of a max-|x| slot: the maximum over its sub-words, as dt_amax_read (dt_internal.h) takes it on the device
extern "C" int dt_amax_read(dt_ctx *ctx, int slot, float *h_out)
{
    if (!ctx || !h_out) return dt_fail(ctx, DT_ERR_ARG, "null argument");
    if (slot < 0 || slot >= DT_AMAX_SLOTS) return dt_fail(ctx, DT_ERR_ARG, "max-|x| slot %d out of range [0, %d)", slot, DT_AMAX_SLOTS);
    if (!ctx->amax) return dt_fail(ctx, DT_ERR_STATE, "max-|x| slots not allocated");
    if (ctx->capturing) return dt_fail(ctx, DT_ERR_STATE, "dt_amax_read during graph capture");
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    unsigned w[DT_AMAX_WORDS];
    HIP_TRY(ctx, hipMemcpy(w, amax_slot(ctx, slot), sizeof(w), hipMemcpyDeviceToHost));
    unsigned v = 0;
    for (int q = 0; q < DT_AMAX_SUB; ++q) v = w[q * DT_AMAX_LINE] > v ? w[q * DT_AMAX_LINE] : v;
    memcpy(h_out, &v, sizeof(v));
    return DT_OK;
}

extern "C" int dt_create(dt_ctx **out)
{
    if (!out) return dt_fail(nullptr, DT_ERR_ARG, "dt_create: null out");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return dt_fail(nullptr, DT_ERR_DEVICE,
                       "dt_create: no HIP device visible -- libmi355_dt has no CPU fallback");
    hipDeviceProp_t prop;
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess)
        return dt_fail(nullptr, DT_ERR_DEVICE, "dt_create: hipGetDeviceProperties failed");
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return dt_fail(nullptr, DT_ERR_DEVICE, "dt_create: device is %s; this library is built for gfx950 only",
                       prop.gcnArchName);
    dt_ctx *c = new dt_ctx();
    policy_refresh(c);
    std::vector<float> lut(256);
    for (int i = 0; i < 256; ++i) lut[i] = (float)((double)i / 255.0);   // utils.py:150-153
    if (upload(c, c->lut255, lut) != DT_OK) {
        snprintf(g_static_err, sizeof(g_static_err), "%s", c->err.c_str());
        delete c;
        return DT_ERR_DEVICE;
    }
    {   // max-|x| slots; slot 0 = 1.0
        std::vector<unsigned> am((size_t)DT_AMAX_SLOTS * DT_AMAX_WORDS, 0u);
        for (int q = 0; q < DT_AMAX_SUB; ++q) am[(size_t)q * DT_AMAX_LINE] = 0x3f800000u;
        if (upload(c, c->amax, am) != DT_OK) {
            snprintf(g_static_err, sizeof(g_static_err), "dt_create: max-|x| slot allocation failed");
            delete c;
            return DT_ERR_DEVICE;
        }
    }
    *out = c;
    return DT_OK;
}

extern "C" void dt_destroy(dt_ctx *ctx)
{
    if (!ctx) return;
    (void)hipStreamSynchronize(ctx->stream);
    for (auto &kv : ctx->ws)
        if (kv.second.p) (void)hipFree(kv.second.p);
    for (auto &e : ctx->pending) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
    if (ctx->gstream) {
        graphs_clear(ctx);
        (void)hipStreamDestroy(ctx->gstream);
    }
    delete ctx;      // every weight buffer goes with its owner (DevMem)
}

extern "C" const char *dt_last_error(dt_ctx *ctx) { return ctx ? ctx->err.c_str() : g_static_err; }

extern "C" int dt_set_stream(dt_ctx *ctx, void *hip_stream)
{
    if (!ctx) return DT_ERR_ARG;
    hipStream_t next = static_cast<hipStream_t>(hip_stream);
    if (next != ctx->stream) {
        // work already queued on the old stream may still use the library's workspaces, and a replayed graph may be in flight there:
        // order the new stream behind it (an event, no host wait), and drop the captured graphs -- graphs_clear() and the workspace
        // grow path synchronise ctx->stream only, which from now on is the new one
        graphs_clear(ctx);                              // (synchronises the OLD stream if any graph exists)
        hipEvent_t ev = nullptr;
        if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) == hipSuccess) {
            if (hipEventRecord(ev, ctx->stream) != hipSuccess || hipStreamWaitEvent(next, ev, 0) != hipSuccess) {
                (void)hipGetLastError();
                (void)hipStreamSynchronize(ctx->stream);      // (e.g. the caller already destroyed the old stream: nothing of it can be in flight then)
            }
            (void)hipEventDestroy(ev);
        } else {
            (void)hipStreamSynchronize(ctx->stream);
        }
        ctx->stream = next;
    }
    return DT_OK;
}

// ---------------------------------------------------------------------------
// stream slots (dt_stream_open): state that outlives a call
// ---------------------------------------------------------------------------
// Every slot fresh again, in stream order: a zero meta row is a fresh slot (the h / c rows of such a slot read as zeros, stream_state.hip).
// The loaders call this: state computed under other weights means nothing.  A table whose rows no longer fit the model is closed.
static int streams_fresh(dt_ctx *ctx)
{
    StreamTable &S = ctx->streams;
    if (!S.n_slots) return DT_OK;
    const int row = (ctx->image_h / 32) * (ctx->image_w / 32) * ctx->trk_units;
    if (row != S.row) {
        (void)hipStreamSynchronize(ctx->stream);
        S = StreamTable();
        return DT_OK;
    }
    HIP_TRY(ctx, hipMemsetAsync(S.meta.get(), 0, (size_t)S.n_slots * STREAM_META * sizeof(int), ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(S.vstamp.get(), 0, (size_t)S.n_slots * sizeof(int), ctx->stream));      // no slot has velocities
    HIP_TRY(ctx, hipMemsetAsync(S.hstamp.get(), 0, (size_t)S.n_slots * sizeof(int), ctx->stream));      // ... nor hit counts
    std::fill(S.warm.begin(), S.warm.end(), 0);
    return DT_OK;
}

// the slot list of a stream call: n distinct numbers in [0, n_slots)
static int streams_check_list(dt_ctx *ctx, const int *h_slots, int n)
{
    const StreamTable &S = ctx->streams;
    if (!S.n_slots) return dt_fail(ctx, DT_ERR_STATE, "dt_stream_open must be called first");
    if (!h_slots || n <= 0 || n > S.n_slots) return dt_fail(ctx, DT_ERR_ARG, "a stream call names between 1 and n_slots = %d slots", S.n_slots);
    std::vector<char> seen((size_t)S.n_slots, 0);
    for (int i = 0; i < n; ++i) {
        if (h_slots[i] < 0 || h_slots[i] >= S.n_slots) return dt_fail(ctx, DT_ERR_ARG, "slot %d is outside [0, %d)", h_slots[i], S.n_slots);
        if (seen[h_slots[i]]) return dt_fail(ctx, DT_ERR_ARG, "slot %d is named twice in one call", h_slots[i]);
        seen[h_slots[i]] = 1;
    }
    return DT_OK;
}

extern "C" int dt_stream_open_tracks(dt_ctx *ctx, int n_slots, int cap, int tcap)
{
    if (!ctx) return DT_ERR_ARG;
    if (!ctx->trk_loaded) return dt_fail(ctx, DT_ERR_STATE, "tracker weights not loaded");
    if (n_slots <= 0 || n_slots > 65535 || cap <= 0) return dt_fail(ctx, DT_ERR_ARG, "n_slots must be in [1, 65535] and cap positive");
    if (tcap < cap || tcap > SM_COUNT_MASK) return dt_fail(ctx, DT_ERR_ARG, "tcap must be in [cap, %d]", (int)SM_COUNT_MASK);
    const long long row = (long long)(ctx->image_h / 32) * (ctx->image_w / 32) * ctx->trk_units;
    if (row <= 0 || row >= (1ll << 31)) return dt_fail(ctx, DT_ERR_ARG, "bad state row size");
    graphs_clear(ctx);      // captured state moves hold the old table's pointers
    (void)hipStreamSynchronize(ctx->stream);
    StreamTable S;
    HIP_TRY(ctx, S.h.alloc((size_t)n_slots * row));
    HIP_TRY(ctx, S.c.alloc((size_t)n_slots * row));
    HIP_TRY(ctx, S.boxes.alloc((size_t)n_slots * tcap * DT_BOX_FLOATS));
    HIP_TRY(ctx, S.ids.alloc((size_t)n_slots * tcap));
    HIP_TRY(ctx, S.ages.alloc((size_t)n_slots * tcap));
    HIP_TRY(ctx, S.vel.alloc((size_t)n_slots * tcap * 2));
    HIP_TRY(ctx, S.vstamp.alloc((size_t)n_slots));
    HIP_TRY(ctx, S.hits.alloc((size_t)n_slots * tcap));
    HIP_TRY(ctx, S.hstamp.alloc((size_t)n_slots));
    HIP_TRY(ctx, S.meta.alloc((size_t)n_slots * STREAM_META));
    HIP_TRY(ctx, S.list.alloc((size_t)n_slots));
    HIP_TRY(ctx, hipMemsetAsync(S.meta.get(), 0, (size_t)n_slots * STREAM_META * sizeof(int), ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(S.vstamp.get(), 0, (size_t)n_slots * sizeof(int), ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(S.hstamp.get(), 0, (size_t)n_slots * sizeof(int), ctx->stream));
    S.n_slots = n_slots; S.cap = cap; S.tcap = tcap; S.row = (int)row;
    S.warm.assign((size_t)n_slots, 0);
    ctx->streams = std::move(S);
    return DT_OK;
}

extern "C" int dt_stream_open(dt_ctx *ctx, int n_slots, int cap)
{
    return dt_stream_open_tracks(ctx, n_slots, cap, cap);
}

extern "C" int dt_stream_reset(dt_ctx *ctx, const int *h_slots, int n)
{
    if (!ctx) return DT_ERR_ARG;
    StreamTable &S = ctx->streams;
    if (!S.n_slots) return dt_fail(ctx, DT_ERR_STATE, "dt_stream_open must be called first");
    if (!h_slots) return streams_fresh(ctx);
    if (n == 0) return DT_OK;
    const int rc = streams_check_list(ctx, h_slots, n);
    if (rc) return rc;
    if (launch_stream_slots(ctx->stream, h_slots, n, S.list.get(), S.meta.get())) return dt_fail(ctx, DT_ERR_DEVICE, "stream reset launch failed");
    // a reset slot's frame counter starts over and would meet an old stamp again: the stamps go with the meta rows
    if (launch_stream_clear_stamps(ctx->stream, S.list.get(), n, S.vstamp.get())) return dt_fail(ctx, DT_ERR_DEVICE, "stream reset launch failed");
    if (launch_stream_clear_stamps(ctx->stream, S.list.get(), n, S.hstamp.get())) return dt_fail(ctx, DT_ERR_DEVICE, "stream reset launch failed");
    for (int i = 0; i < n; ++i) S.warm[h_slots[i]] = 0;
    return DT_OK;
}

// ---------------------------------------------------------------------------
// detector
// ---------------------------------------------------------------------------
extern "C" int dt_detector_config(dt_ctx *ctx, int image_h, int image_w, int nb_box, int nb_class,
                                  const float *h_anchors)
{
    if (!ctx) return DT_ERR_ARG;
    if (image_h <= 0 || image_w <= 0 || image_h % 32 || image_w % 32)
        return dt_fail(ctx, DT_ERR_ARG, "image size %dx%d must be a positive multiple of 32", image_h, image_w);
    if (nb_box <= 0 || nb_box > 32 || nb_class <= 0 || !h_anchors)
        return dt_fail(ctx, DT_ERR_ARG, "bad nb_box/nb_class/anchors");
    ctx->image_h = image_h; ctx->image_w = image_w;
    ctx->cb = nb_box * (5 + nb_class);
    ctx->det_loaded = false;
    return streams_fresh(ctx);
}

// kernel in the darknet file is (O,I,H,W) (KerasYOLO.py:267-268 reshapes the
// reversed Keras shape and transposes [2,3,1,0]) -> HWIO
static void oihw_to_hwio(const float *src, int O, int I, int k, std::vector<float> &dst)
{
    dst.resize((size_t)O * I * k * k);
    for (int o = 0; o < O; ++o)
        for (int i = 0; i < I; ++i)
            for (int y = 0; y < k; ++y)
                for (int x = 0; x < k; ++x)
                    dst[(((size_t)y * k + x) * I + i) * O + o] = src[(((size_t)o * I + i) * k + y) * k + x];
}

// Policy::wino: 1 (default) = layers with Cin >= 64 and Cout >= 128 (conv_3 and up: below that the batched
//          GEMMs have K <= 32 and the transforms' traffic costs more than the MFMA work saved) when a
//          launch has enough tiles (wino_runs);
//          0 = never (direct MFMA form everywhere); 2 = every 3x3 layer the transforms support,
//          at any size (parity tests of the path at small shapes).  Applied when weights are loaded.
static bool wino_wanted(const dt_ctx *ctx, int ks, int cin, int cout)
{
    const Policy &p = ctx->pol;
    if (ks != 3 || p.wino == 0 || cin % 32 || cout % 4) return false;
    return p.wino == 2 || (cin >= 64 && cout >= 128);
}

// Output tile of the Winograd form: 6 = F(6x6,3x3) (default), 4 = F(4x4,3x3), 2 = F(2x2,3x3); Policy::wino_tile
// forces one size for every layer.  Applied when weights are loaded.
static int wino_tile(const dt_ctx *ctx, bool recurrent)
{
    // The ConvLSTM recurrent convolution keeps F(4x4): its per-step GEMM has only clips/4 * 49 rows, which F(6x6)
    // (clips/9 * 49) fills no better, and the F(6x6) gate-update transform needs all 256 VGPRs (2.0 vs 5.3 TB/s).
    const int t = ctx->pol.wino_tile ? ctx->pol.wino_tile : (recurrent ? 4 : 6);
    return (t == 2 || t == 4) ? t : 6;
}

// One Winograd weight set: U in fp32 and, where the caller's GEMM can take the split kernel, its 16-bit forms (split on the device from the fp32
// copy).  Built aside and moved into `dst` when every step succeeded: a failed upload leaves `dst` as it was.
static int upload_wino(dt_ctx *ctx, WinoWeights &dst, int ts, const float *hwio, int cin_src, int cout_src, const int *cin_map,
                       int cin_dst, const int *n_map, int npad, const float *scale, bool want_s3)
{
    const int P = (ts + 2) * (ts + 2);
    std::vector<float> u((size_t)P * npad * cin_dst);
    wino_pack_weights(ts, hwio, cin_src, cout_src, cin_map, cin_dst, n_map, npad, scale, u.data());
    WinoWeights w;
    w.ts = ts; w.cin = cin_dst; w.npad = npad;
    const int rc = upload(ctx, w.u, u);
    if (rc) return rc;
    // the split-bf16 form of wino_gemm_s3.hip -- only where run_wino can use it: F(6x6) weights of a plain layer, F(4x4) weights of the
    // ConvLSTM recurrent convolution (the caller says which)
    if (want_s3 && ctx->pol.s3 != 0 && cin_dst % 32 == 0 && npad % 128 == 0) {
        HIP_TRY(ctx, w.s3.alloc(u.size() * 3));
        if (launch_wino_s3_pack(ctx->stream, w.u.get(), P, npad, cin_dst, w.s3.get()) || hipStreamSynchronize(ctx->stream) != hipSuccess)
            return dt_fail(ctx, DT_ERR_DEVICE, "split-bf16 weight pack failed");
        if (ctx->pol.s3_h2 != 0 && P <= 64) {      // ... and the fp16 form next to it (DT_PIN runs take the bf16 one)
            HIP_TRY(ctx, w.h2.alloc(u.size() * 2));
            HIP_TRY(ctx, w.h2_pscale.alloc(P));
            if (launch_wino_h2_pack(ctx->stream, w.u.get(), P, npad, cin_dst, ts, amax_slot(ctx, AMAX_PACK), w.h2.get(), w.h2_pscale.get()) ||
                hipStreamSynchronize(ctx->stream) != hipSuccess)
                return dt_fail(ctx, DT_ERR_DEVICE, "fp16-form weight pack failed");
        }
    }
    dst = std::move(w);
    return DT_OK;
}

static void gate_interleave_map(int U, std::vector<int> &n_map)
{
    // packed column n' = (j/32)*128 + g*32 + j%32  <-  Keras column g*U + j
    n_map.resize((size_t)4 * U);
    for (int np = 0; np < 4 * U; ++np) {
        const int jb = np / 128, g = (np % 128) / 32, jj = np % 32;
        n_map[np] = g * U + jb * 32 + jj;
    }
}

// Every device form of one layer's weights, built into a fresh ConvLayer that replaces ctx->layers[idx] when all of it succeeded.
static int load_conv_layer(dt_ctx *ctx, int idx, int ks, int cin, int cout, const float *hwio, const float *scale,
                           const float *bias_src)
{
    ConvLayer L;
    L.idx = idx; L.ks = ks; L.cin = cin; L.cout = cout;
    L.npad = round_up(cout, 256);   // weight rows padded to the widest column tile (256)
    std::vector<float> packed((size_t)L.npad * ks * ks * cin);
    pack_conv_weights(hwio, ks, cin, cout, nullptr, cin, nullptr, L.npad, scale, packed.data());
    std::vector<float> bias(L.npad, 0.0f);
    for (int c = 0; c < cout; ++c) bias[c] = bias_src[c];
    int rc = upload(ctx, L.wt, packed);
    if (rc) return rc;
    if (ks == 1 && ctx->pol.s3 != 0 && ctx->pol.s3_1x1 != 0 && cin % 32 == 0 && L.npad % 128 == 0 && cout >= 64) {
        // a 1x1 layer's weights are a plain [npad][cin] matrix: also as the split-bf16 B operand of wino_gemm_s3.hip
        HIP_TRY(ctx, L.wt_s3.alloc(packed.size() * 3));
        if (launch_wino_s3_pack(ctx->stream, L.wt.get(), 1, L.npad, cin, L.wt_s3.get())) return dt_fail(ctx, DT_ERR_DEVICE, "split-bf16 weight pack launch failed");
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        // the bias as one extra K stage (wino_gemm_s3.hip): B rows (bias[n], 0, .., 0), A rows (1, 0, .., 0)
        std::vector<unsigned short> bs((size_t)3 * L.npad * 16, 0);
        for (int n = 0; n < cout; ++n) {
            unsigned short t[3];
            wino_s3_split_host(bias_src[n], t);
            for (int t3 = 0; t3 < 3; ++t3) bs[((size_t)t3 * L.npad + n) * 16] = t[t3];
        }
        if ((rc = upload(ctx, L.bias_s3, bs))) return rc;
        if (!ctx->s3_ones) {
            std::vector<float> ones((size_t)256 * 16, 0.0f);      // the bias stage's A rows, fp32 like the layer's activation: (1, 0, .., 0)
            for (int r = 0; r < 256; ++r) ones[(size_t)r * 16] = 1.0f;
            if ((rc = upload(ctx, ctx->s3_ones, ones))) return rc;
        }
    }
    if (L.wt_s3 && ctx->pol.s3_h2 != 0) {
        // ... and in the fp16 form: two terms of wt * 2^s (s from max |wt|), the epilogue factor 2^-s; the bias stays fp32 (L.bias)
        HIP_TRY(ctx, L.wt_h2.alloc(packed.size() * 2));
        HIP_TRY(ctx, L.pscale_h2.alloc(1));
        if (launch_wino_h2_pack(ctx->stream, L.wt.get(), 1, L.npad, cin, 0, amax_slot(ctx, AMAX_PACK), L.wt_h2.get(), L.pscale_h2.get()))
            return dt_fail(ctx, DT_ERR_DEVICE, "fp16-form weight pack launch failed");
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    if (ks == 3 && (cin == 32 || cin == 64) && cout % 64 == 0 && cout <= 128 && ctx->pol.s3 != 0 && ctx->pol.s3_h2 != 0 && ctx->pol.c3h2 != 0) {
        // conv_2 / conv_3 / conv_5's shapes: the packed direct-form weights as two fp16 terms for conv3_h2.hip (the same k order)
        HIP_TRY(ctx, L.w3_h2.alloc(packed.size() * 2));
        HIP_TRY(ctx, L.pscale_w3.alloc(1));
        if (launch_wino_h2_pack(ctx->stream, L.wt.get(), 1, L.npad, 9 * cin, 0, amax_slot(ctx, AMAX_PACK), L.w3_h2.get(), L.pscale_w3.get()))
            return dt_fail(ctx, DT_ERR_DEVICE, "fp16-form weight pack launch failed");
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    if (scale) {
        std::vector<float> sc(scale, scale + cout);
        for (float v : sc) L.scale_has_zero |= (v == 0.0f);
        if ((rc = upload(ctx, L.scale, sc))) return rc;
    }
    const bool f4_shape = ((cin == 64 || cin == 128) && cout % 128 == 0 && cout <= 256) || (cin == 32 && cout == 64);
    if (ks == 3 && f4_shape && ctx->pol.wino != 0 && ctx->pol.fused4 != 0) {
        // conv_2 / conv_3 / conv_5 / conv_6 / conv_8's shapes: the fused F(4x4,3x3) kernel (wino4s_fused.hip)
        std::vector<float> u36((size_t)36 * L.npad * cin), uf((size_t)36 * cin * cout);
        wino_pack_weights(4, hwio, cin, cout, nullptr, cin, nullptr, L.npad, scale, u36.data());
        wino4s_fused_pack(u36.data(), L.npad, cin, cout, uf.data());
        if ((rc = upload(ctx, L.fused4s, uf))) return rc;
    }
    if (wino_wanted(ctx, ks, cin, cout)) {
        const int ts = wino_tile(ctx, false);
        rc = upload_wino(ctx, L.wino, ts, hwio, cin, cout, nullptr, cin, nullptr, L.npad, scale, ts == 6);
        if (rc) return rc;
        // small batches of the 13x13 / 26x26 layers: F(4x4) needs 36 GEMMs of ONE (partly filled) row tile where F(6x6)
        // needs 64 -- keep both weight sets and choose per launch (run_conv); only with the default tile policy
        if (ts == 6 && ctx->pol.wino_tile == 0 && cin >= 256) {
            rc = upload_wino(ctx, L.wino_alt, 4, hwio, cin, cout, nullptr, cin, nullptr, L.npad, scale, false);
            if (rc) return rc;
        }
    }
    if ((rc = upload(ctx, L.bias, bias))) return rc;
    (void)hipStreamSynchronize(ctx->stream);      // the layer this one replaces may still be read by queued work
    ctx->layers[idx] = std::move(L);
    return DT_OK;
}

// The ConvLSTM2D input projection with conv_23 folded in (Policy::trk_merge).  z = [x_bbox | conv_feat] with x_bbox = W23 feat + b23 inside
// the image (conv_23 is a 1x1 convolution with a LINEAR activation, KerasYOLO.py:396-400) and zero in the 'same' padding, so
//     Wx * z + b  =  (Wx[feat] + W23 Wx[bbox]) * feat  +  b  +  sum over the taps INSIDE the image of  b23 . Wx[bbox][tap]
// -- one 3x3 convolution of conv_feat alone (K = 1024 instead of 1109 -> 1120) with a bias that depends on which of its nine taps lie
// inside the image (16 border cases).  Merged in float64 on the host whenever both weight sets are present; used by the Winograd path
// of the projection (convlstm_sequence), the two-step form stays for the small-batch direct path and for DT_TRK_MERGE=0.
static int build_merged_xproj(dt_ctx *ctx)
{
    (void)hipStreamSynchronize(ctx->stream);      // queued work may still read the set this one replaces
    ctx->trk_wxm_wino = WinoWeights();
    ctx->trk_bx16.reset();
    const int Cb = ctx->cb, U = ctx->trk_units, N4 = 4 * U, Csrc = Cb + 1024;
    if (!ctx->pol.trk_merge || !U || ctx->conv23_hwio.size() != (size_t)1024 * Cb || ctx->trk_hkernel.size() != (size_t)9 * Csrc * N4) return DT_OK;
    // (F(6x6) only, and not next to an unmerged set that was built with another tile: one tile for both forms of the projection)
    if (!wino_wanted(ctx, 3, 1024, N4) || wino_tile(ctx, false) != 6 || (ctx->trk_wx_wino.u && ctx->trk_wx_wino.ts != 6)) return DT_OK;
    const float *wk = ctx->trk_hkernel.data(), *w23 = ctx->conv23_hwio.data();
    std::vector<float> merged((size_t)9 * 1024 * N4);
    {   // 9 x 1024 independent rows of Cb x 4U float64 multiply-adds (1.6 G at C = 12): over the host's threads
        auto work = [&](int r0, int r1) {
            std::vector<double> row(N4);
            for (int r = r0; r < r1; ++r) {
                const int tap = r / 1024, c = r % 1024;
                const float *src = wk + ((size_t)tap * Csrc + Cb + c) * N4;           // Keras input order: x_bbox first, then conv_feat
                for (int n = 0; n < N4; ++n) row[n] = src[n];
                for (int j = 0; j < Cb; ++j) {
                    const double a = w23[(size_t)c * Cb + j];
                    const float *wb = wk + ((size_t)tap * Csrc + j) * N4;
                    for (int n = 0; n < N4; ++n) row[n] += a * wb[n];
                }
                float *dst = merged.data() + ((size_t)tap * 1024 + c) * N4;
                for (int n = 0; n < N4; ++n) dst[n] = (float)row[n];
            }
        };
        unsigned nth = std::thread::hardware_concurrency();
        nth = nth < 1 ? 1 : (nth > 16 ? 16 : nth);
        std::vector<std::thread> pool;
        for (unsigned i = 0; i < nth; ++i) pool.emplace_back(work, (int)(9216ull * i / nth), (int)(9216ull * (i + 1) / nth));
        for (auto &th : pool) th.join();
    }
    std::vector<int> n_map;
    gate_interleave_map(U, n_map);
    // bias of border case k: b + sum over the taps (dy, dx) whose pixel exists: dy = 0 needs h > 0, dy = 2 needs h < H - 1, likewise dx
    std::vector<double> tapb((size_t)9 * N4, 0.0);
    for (int tap = 0; tap < 9; ++tap)
        for (int j = 0; j < Cb; ++j) {
            const double bj = ctx->conv23_bias[j];
            const float *wb = wk + ((size_t)tap * Csrc + j) * N4;
            for (int n = 0; n < N4; ++n) tapb[(size_t)tap * N4 + n] += bj * wb[n];
        }
    // row 0: the interior bias (all nine taps); row 1 + k: what border case k takes away from it (the taps outside the image), as a correction
    std::vector<float> b16((size_t)17 * N4);
    for (int k = 0; k < 16; ++k)
        for (int np = 0; np < N4; ++np) {
            const int n = n_map[np];
            double all = ctx->trk_hbias[n], out = 0.0;
            for (int dy = 0; dy < 3; ++dy)
                for (int dx = 0; dx < 3; ++dx) {
                    const bool in = !(dy == 0 && (k & 1)) && !(dy == 2 && (k & 2)) && !(dx == 0 && (k & 4)) && !(dx == 2 && (k & 8));
                    all += tapb[(size_t)(dy * 3 + dx) * N4 + n];
                    if (!in) out += tapb[(size_t)(dy * 3 + dx) * N4 + n];
                }
            if (k == 0) b16[np] = (float)all;
            b16[(size_t)(1 + k) * N4 + np] = (float)(-out);
        }
    int rc = upload_wino(ctx, ctx->trk_wxm_wino, 6, merged.data(), 1024, N4, nullptr, 1024, n_map.data(), N4, nullptr, true);
    if (rc) return rc;
    return upload(ctx, ctx->trk_bx16, b16);
}

// conv_1's weights [27][32] (BatchNorm scale folded) as three bf16 terms, plain (float32 frames) and with normalize()'s 1/255 folded in (uint8
// frames): conv1_s3_kernel's tables, each 1536 words + 4 zero words (the kernel's source of padding pixels).  dt_load_darknet_weights and dt_conv1.
static int upload_conv1_tables(dt_ctx *ctx, const float *w, DevMem<unsigned> &d_w3, DevMem<unsigned> &d_w3u8)
{
    std::vector<unsigned> w3(C1_W3_WORDS, 0u), w3u8(C1_W3_WORDS, 0u);
    conv1_split_tables(w, false, w3.data());
    conv1_split_tables(w, true, w3u8.data());
    int rc;
    if ((rc = upload(ctx, d_w3, w3)) || (rc = upload(ctx, d_w3u8, w3u8))) return rc;
    return DT_OK;
}

extern "C" int dt_load_darknet_weights(dt_ctx *ctx, const float *h_blob, size_t n_floats, size_t *consumed)
{
    if (!ctx || !h_blob) return DT_ERR_ARG;
    if (!ctx->cb) return dt_fail(ctx, DT_ERR_STATE, "dt_detector_config must be called first");
    size_t off = 4;   // WeightReader.offset = 4 (utils.py:140)
    auto take = [&](size_t n) -> const float * {
        if (off + n > n_floats) return nullptr;
        const float *p = h_blob + off;
        off += n;
        return p;
    };
    struct Spec { int idx, k, cin, cout; };
    std::vector<Spec> specs;
    for (auto &t : TRUNK) specs.push_back({t[0], t[1], t[2], t[3]});
    specs.push_back({21, 1, 512, 64});
    specs.push_back({22, 3, 1280, 1024});
    std::vector<float> hwio, scale, shift;
    for (const Spec &s : specs) {   // file order conv_1 .. conv_22, each: beta, gamma, mean, var, kernel
        const float *beta = take(s.cout), *gamma = take(s.cout), *mean = take(s.cout), *var = take(s.cout);
        const float *kern = take((size_t)s.cout * s.cin * s.k * s.k);
        if (!kern) return dt_fail(ctx, DT_ERR_ARG, "weights blob too short at conv_%d", s.idx);
        scale.resize(s.cout); shift.resize(s.cout);
        for (int c = 0; c < s.cout; ++c) {
            scale[c] = gamma[c] * (1.0f / sqrtf(var[c] + BN_EPS));
            shift[c] = beta[c] - mean[c] * scale[c];
        }
        oihw_to_hwio(kern, s.cout, s.cin, s.k, hwio);
        if (s.idx == 1) {   // direct kernel layout [27][32]
            std::vector<float> w(27 * 32);
            for (int t = 0; t < 27; ++t)
                for (int c = 0; c < 32; ++c) w[t * 32 + c] = hwio[(size_t)t * 32 + c] * scale[c];
            (void)hipStreamSynchronize(ctx->stream);      // queued work may still read the tables these replace
            int rc;
            if ((rc = upload(ctx, ctx->conv1_w, w)) || (rc = upload(ctx, ctx->conv1_b, shift)) ||
                (rc = upload_conv1_tables(ctx, w.data(), ctx->conv1_w3, ctx->conv1_w3u8)))
                return rc;
            ctx->conv1_hwio32.assign((size_t)9 * 32 * 32, 0.0f);   // [3][3][32 (3 used)][32]
            for (int t = 0; t < 9; ++t)
                for (int ci = 0; ci < 3; ++ci)
                    for (int c = 0; c < 32; ++c)
                        ctx->conv1_hwio32[((size_t)t * 32 + ci) * 32 + c] = hwio[((size_t)t * 3 + ci) * 32 + c];
            ctx->conv1_scale = scale; ctx->conv1_shift = shift;
        } else {
            int rc = load_conv_layer(ctx, s.idx, s.k, s.cin, s.cout, hwio.data(), scale.data(), shift.data());
            if (rc) return rc;
        }
    }
    {   // conv_23: bias then kernel, no BN (KerasYOLO.py:264-269)
        const int co = ctx->cb;
        const float *bias = take(co);
        const float *kern = take((size_t)co * 1024);
        if (!kern) return dt_fail(ctx, DT_ERR_ARG, "weights blob too short at conv_23");
        oihw_to_hwio(kern, co, 1024, 1, hwio);
        int rc = load_conv_layer(ctx, 23, 1, 1024, co, hwio.data(), nullptr, bias);
        if (rc) return rc;
        ctx->conv23_hwio.assign(hwio.begin(), hwio.begin() + (size_t)1024 * co);      // [1024][co]
        ctx->conv23_bias.assign(bias, bias + co);
    }
    if (consumed) *consumed = off;
    graphs_clear(ctx);
    ctx->det_loaded = true;
    if (const int rc = streams_fresh(ctx)) return rc;
    return build_merged_xproj(ctx);
}

// Direct-form FLOPs (2*M*K*N of the reference's convolution) and bytes (in + weights + out, fp32) of every layer, booked
// under the kernel FAMILY whose launch computed it -- "conv_direct_form" (conv_igemm_f32 launches), "conv_direct_form_s3"
// (wino_gemm_s3 launches), "conv_direct_form_fused" (the fused Winograd kernel) -- so that bench.py divides each family's
// algorithmic work by that family's own time and no family is credited with work another kernel did.
enum { DF_IGEMM = 0, DF_FUSED = 1, DF_S3 = 2, DF_CONV1 = 3, DF_C3H2 = 4 };
static const char *const k_direct_form[] = {"conv_direct_form", "conv_direct_form_fused", "conv_direct_form_s3", "conv_direct_form_conv1", "conv_direct_form_c3h2"};
static void prof_direct_form(dt_ctx *ctx, double flops, double bytes, int family = DF_IGEMM)
{
    if (!ctx->prof) return;
    ProfEntry &e = ctx->prof_tab[k_direct_form[family]];
    e.flops += flops;
    e.bytes += bytes;   // in + weights + out of the reference's layer, float32
}

// ---------------------------------------------------------------------------
// Winograd path for the 3x3 layers from conv_3 up and the ConvLSTM convolutions (winograd.hip)
// ---------------------------------------------------------------------------
// Thresholds the A/B rounds settled (profiles/r04_experiments.txt, r06_experiments.txt).  The split GEMM (wino_gemm_s3.hip) from K = 128
// (round 4: with the line-sized epilogue stores the K = 128 GEMMs of conv_6 / conv_8 take 3.4 instead of 4.3 ms on the fp32 kernel, their
// split input transform costs 0.7 back):
static const int S3_MINK = 128;
// blocks of 16 x 16 pixels from which a narrow 3x3 layer (conv_2 / 3 / 5) takes the direct fp16-form kernel (conv3_h2.hip) instead of the fused fp32 one:
static const long long C3H2_MIN_BLOCKS = 1024;

static bool wino_runs(const dt_ctx *ctx, const WinoWeights &wts, int B, int H, int W, int N)
{
    if (!wts.u) return false;
    const int ts = wts.ts, cin = wts.cin;
    const long long mt = (long long)B * ((H + ts - 1) / ts) * ((W + ts - 1) / ts);
    if (mt >= (1ll << 31) / 64) return false;
    // V and M' workspaces are (ts+2)^2 * tiles * (Cin + N) floats (27 GB for conv_3 at 1440 frames); a launch
    // that would need more than Policy::wino_ws_gb (default 96) takes the direct form instead of failing to allocate
    if (4.0 * (ts + 2) * (ts + 2) * (double)mt * ((double)cin + N) > ctx->pol.wino_ws_gb * 1e9) return false;
    // below this many tiles the batched GEMMs' row tiles are mostly empty and the direct (split-K) form wins
    // (detector-only sweep, batch 1/4/8/16: threshold 512 -> 679/1822/2672/3487 frames/s, 64 -> 695/1960/3341/4402,
    // 16 -> 556/1947/3337/4427)
    const int mint = ctx->pol.wino_mint;
    // (F(4x4) -- the ConvLSTM recurrent step -- from 16 tiles = ONE clip at 13x13 since round 6: with the step's GEMM on the split kernel a 30-frame clip takes 4.7 instead
    //  of 12.3 ms, two clips 6.5 instead of 14.3, three 7.7 instead of 15.7 (profiles/r06_experiments.txt section 10); on the fp32 kernel too the Winograd form wins there)
    return ctx->pol.wino == 2 || mt >= (mint > 0 ? mint : (ts == 2 ? 256 : (ts == 4 ? 16 : 32)));
}

// Tile configuration of the P batched GEMMs [Mt x Cin] x [Cin x N] (persistent launch, conv_igemm.hip).
// Measured (tools/wino_ab.sh): a GEMM tile is only Cin/32 = 4..40 chunks long, so what matters is what
// happens BETWEEN tiles.  One tile per workgroup: 128x128 (two workgroups per CU overlap each other's
// epilogue/prologue) 128.6 vs 256x256 121.4 TFLOP/s at K=1024.  Persistent with the next tile's first DMA
// issued inside the last chunk: 256x256 132.4 (K=1024), 128.3 (K=512), 122.3 (K=256) -- ahead of 128x128
// everywhere, so the wide tile is taken whenever wave quantisation does not eat the gain.
// Small batched GEMMs (a few frames per call): what counts is the busiest CU.  cost = rounds over the 256 CUs x tile
// area / relative efficiency of the tile shape, in units of one 128x128 tile of this K (measured at batch 8,
// tools/batch8_layers.py: the 13x13 layers' F(4x4) GEMMs as 36 x 8 tiles of 128x128 leave 224 CUs with one tile and 32
// with two -- 139 us; as 36 x 16 tiles of 128x64: 112 us; as F(6x6) with 64 x 8 tiles of 64x128 (50 Winograd tiles fit
// one 64-row tile): 81 us).  Returns the cheapest shape and its cost.
static double small_gemm_cost(int Mt, int N, int P, int *cfg_out)
{
    const long long t128 = (long long)P * ((Mt + 127) / 128) * ((N + 127) / 128);
    const long long t64n = (long long)P * ((Mt + 127) / 128) * ((N + 63) / 64);
    const long long t64m = (long long)P * ((Mt + 63) / 64) * ((N + 127) / 128);
    const long long t256 = (long long)P * ((Mt + 255) / 256) * ((N + 255) / 256);
    double best = (double)((t128 + 255) / 256);
    int cfg = CFG_128x128;
    const double c64n = N % 64 == 0 ? (double)((t64n + 255) / 256) * 0.5 / 0.92 : 1e30;
    const double c64m = (double)((t64m + 255) / 256) * 0.5 / 0.92;
    const double c256 = N % 256 == 0 ? (double)((t256 + 255) / 256) * 4.0 / 1.03 : 1e30;
    if (c64n < best) { best = c64n; cfg = CFG_128x64; }
    if (c64m < best) { best = c64m; cfg = CFG_64x128; }
    if (c256 < best) { best = c256; cfg = CFG_256x256; }
    if (cfg_out) *cfg_out = cfg;
    return best;
}

static int pick_cfg_gemm(int Mt, int N, int P)
{
    const long long t128 = (long long)P * ((Mt + 127) / 128) * ((N + 127) / 128);
    if (t128 <= 4096) {
        int cfg;
        (void)small_gemm_cost(Mt, N, P, &cfg);
        return cfg;
    }
    if (N % 256 == 0) {
        const long long t256 = (long long)P * ((Mt + 255) / 256) * (N / 256);
        const double e256 = (double)Mt / (((Mt + 255) / 256) * 256.0) * (double)t256 / (double)(((t256 + 255) / 256) * 256);
        const double e128 = (double)Mt / (((Mt + 127) / 128) * 128.0) * (double)t128 / (double)(((t128 + 511) / 512) * 512);
        if (e256 * 1.03 > e128) return CFG_256x256;
    }
    return CFG_128x128;
}

// every MFMA-kernel launch of this file goes through here: the context's forced tile configuration (tests, A/B) rides along
static int launch_igemm(dt_ctx *ctx, ConvArgs &a, int ks, int order, int epi, int cfg)
{
    a.force_cfg = ctx->pol.conv_cfg >= 0 ? ctx->pol.conv_cfg + 1 : 0;
    return launch_conv_igemm(ctx->stream, a, ks, order, epi, cfg);
}

struct WinoIO {
    const float *in; long long in_bs; int in_ld;      // NHWC input
    float *out; long long out_bs; int out_ld;         // full-resolution output (null: pooled only)
    float *out2; int out2_ld;                         // 2x2 pooled output or null
    const float *xproj; long long xp_bs; int xp_ld;   // gates variant (cstate != null)
    float *cstate; long long c_bs; int c_ld;
    const float *bias16;                              // border-aware bias [16][N] instead of `bias` (WinoArgs::bias16) or null
    unsigned *amax_out;                               // the output transform takes max |x| of what it stores into this slot, or null (the caller tags the tensor)
};

// Tile geometry of a Winograd launch.  Mosaic factor g: g x g frames with zero separators share one virtual image
// (winograd.hip:vpixel) when that needs fewer tiles per frame (13x13 F(4x4): 12.25 instead of 16).  The frame pitch ph / pw
// belongs to the launch: H + 1 / W + 1 (one separator), and the next EVEN number where the launch pools, so that frame and
// tile origins are even and no 2x2 pooling window straddles a tile or a frame (winograd.hip:pooled_pixel).  g runs to 6:
//   13x13 F(6x6): g = 3, 42 = 7 tiles, 5.44 per frame (9);   26x26: g = 2, 54 = 9 tiles, 20.25 (25);   13x13 F(4x4): g = 2, 28 = 7 tiles, 12.25 (16);
//   26x26 pooled (conv_13): pitch 28, g = 3, 84 = 14 tiles, 21.78 (25);   52x52 (conv_6): pitch 53, g = 6, 318 = 53 tiles, 78.03 (81);
//   52x52 pooled (conv_8): pitch 54 = 9 tiles for every g: stays at 81.
// The rule prices whole groups: a ragged last group costs a whole mosaic's tiles (B >= g * g keeps it to a factor below 2).
struct WinoGeom { int g, ph, pw, th, tw, Mt; };
static WinoGeom wino_geometry(const dt_ctx *ctx, int ts, int B, int H, int W, bool pooled)
{
    WinoGeom q;
    q.g = 1;
    q.ph = pooled ? (H + 2) & ~1 : H + 1;
    q.pw = pooled ? (W + 2) & ~1 : W + 1;
    const int g_env = ctx->pol.mosaic;   // 1: never (tests, A/B), 2 .. 6: force
    double best = (double)((H + ts - 1) / ts) * ((W + ts - 1) / ts);
    for (int g = 2; g <= 6 && g_env != 1; ++g) {
        const double t = (double)((g * q.ph + ts - 1) / ts) * ((g * q.pw + ts - 1) / ts) / (g * g);
        if ((t < best * 0.97 && B >= g * g) || g_env == g) { best = t; q.g = g; }
    }
    if (q.g == 1) { q.th = (H + ts - 1) / ts; q.tw = (W + ts - 1) / ts; q.Mt = B * q.th * q.tw; }
    else {
        q.th = (q.g * q.ph + ts - 1) / ts; q.tw = (q.g * q.pw + ts - 1) / ts;
        q.Mt = ((B + q.g * q.g - 1) / (q.g * q.g)) * q.th * q.tw;
    }
    return q;
}

// What a launch leaves behind, from its epilogue: the range(s) it overwrites (the pooled epilogues write a quarter of the pixels; the s2d epilogue a quarter with 4x
// the row) -- amax_forget before the launch -- and among them the tensor the next layer reads, lo[next] with `cols` channels per pixel -- amax_note after a launch that
// publishes: pooled where the epilogue pools (the unpooled twin of conv_13 feeds conv_21's fp32 kernel), 4 N channels per quarter-resolution pixel after space_to_depth.
struct Leaves { const float *lo[2]; long long floats[2]; int next, cols; };
static Leaves conv_leaves(int epi, const float *out, int out_ld, const float *out2, int out2_ld, long long M, int cout)
{
    return Leaves{{out, out2}, {(epi == EPI_POOL || epi == EPI_S2D ? M / 4 : M) * out_ld, out2 ? M / 4 * out2_ld : 0}, epi == EPI_POOL_BOTH ? 1 : 0,
                  epi == EPI_S2D ? 4 * cout : cout};
}
static void amax_forget(dt_ctx *ctx, const Leaves &lv) { amax_forget(ctx, lv.lo[0], lv.floats[0]); amax_forget(ctx, lv.lo[1], lv.floats[1]); }
static void amax_note(dt_ctx *ctx, const Leaves &lv, int slot) { amax_note(ctx, lv.lo[lv.next], lv.floats[lv.next], lv.cols, slot); }

// The form of one Winograd launch: its tile geometry and the kernel its batched GEMMs take -- nt = 0: the fp32 MFMA kernel; 3 / 2: the split GEMM
// (wino_gemm_s3.hip) with three bf16 / two fp16 terms per operand.  Decided here and nowhere else; run_wino launches what it is handed.
struct WinoChoice { WinoGeom q; int nt; };
static WinoChoice choose_wino(const dt_ctx *ctx, const WinoWeights &wts, int N, int B, int H, int W, bool pooled, bool gates)
{
    const int ts = wts.ts, cin = wts.cin;
    WinoChoice c{wino_geometry(ctx, ts, B, H, W, pooled), 0};
    // the GEMMs on the bf16 pipe with split operands (wino_gemm_s3.hip) where that form exists and wins: long K, enough rows
    const bool rec = ts == 4 && gates;      // the recurrent step: F(4x4), gate update in the output transform
    // (row thresholds: the fp16 form wins from far fewer rows than the bf16 form)
    const bool h2_avail = h2_wanted(ctx) && wts.h2;
    const int minrows = h2_avail ? ctx->pol.s3_minrows_h2 : ctx->pol.s3_minrows, rec_minrows = h2_avail ? ctx->pol.s3_rec_minrows_h2 : ctx->pol.s3_rec_minrows;
    if (((ts == 6 && !gates) || rec) && ctx->pol.s3 != 0 && cin % 32 == 0 && N % 128 == 0 && wts.npad % 128 == 0 && wino_gemm_s3_usable(c.q.Mt, cin, N) &&
        (ctx->pol.s3 == 2 || (cin >= S3_MINK && (rec ? (rec_minrows > 0 && c.q.Mt >= rec_minrows) : c.q.Mt >= minrows))) && wts.s3)
        c.nt = h2_avail ? 2 : 3;      // ... in the fp16 form (two terms of scaled operands, three products) where its weights exist
    return c;
}
static WinoChoice choose_wino(const dt_ctx *ctx, const WinoWeights &wts, int N, int B, int H, int W, const WinoIO &io) { return choose_wino(ctx, wts, N, B, H, W, io.out2 != nullptr, io.cstate != nullptr); }

static int run_wino(dt_ctx *ctx, const WinoWeights &wts, const WinoChoice &wc, const float *bias, int N, int B, int H, int W, const WinoIO &io, float slope,
                    const char *tag, int cin_alg = 0 /* channels of the reference's layer when cin is padded */,
                    int in_slot = AMAX_TEST /* max-|x| slot of the input tensor (fp16 form); AMAX_ONE: bounded by 1, nothing to measure */)
{
    const int ts = wts.ts, cin = wts.cin, npad = wts.npad;
    const double cin_df = cin_alg > 0 ? cin_alg : cin;
    amax_forget(ctx, io.out ? conv_leaves(io.out2 ? EPI_POOL_BOTH : EPI_PLAIN, io.out, io.out_ld, io.out2, io.out2_ld, (long long)B * H * W, N)
                            : conv_leaves(EPI_POOL, io.out2, io.out2_ld, nullptr, 0, (long long)B * H * W, N));
    WinoArgs w{};
    w.B = B; w.H = H; w.W = W; w.ts = ts;
    w.g = wc.q.g; w.ph = wc.q.ph; w.pw = wc.q.pw; w.th = wc.q.th; w.tw = wc.q.tw; w.Mt = wc.q.Mt;
    prof_count(ctx, "wino_mosaic:g%d_ts%d", w.g, ts);   // which mosaic / tile size a launch took
    const int P = (ts + 2) * (ts + 2);
    const size_t mt = (size_t)w.Mt;
    const bool h2 = wc.nt == 2;
    const unsigned short *u_s3 = h2 ? wts.h2.get() : (wc.nt == 3 ? wts.s3.get() : nullptr);
    const int NT = h2 ? 2 : 3;
    const size_t mp = (mt + 255) / 256 * 256;
    float *V = ws_get(ctx, "wino_v", u_s3 ? (size_t)P * NT * mp * cin * sizeof(unsigned short) : P * mt * cin * sizeof(float));
    float *Mp = ws_get(ctx, "wino_m", P * mt * N * sizeof(float));
    if (!V || !Mp) return DT_ERR_DEVICE;
    if (u_s3) { w.v_s3 = reinterpret_cast<unsigned short *>(V); w.Mp = (int)mp; }
    const unsigned *amax = nullptr;
    if (h2) {      // V's power of two comes from the input's max |x|
        amax = in_slot == AMAX_ONE ? amax_slot(ctx, AMAX_ONE) : ensure_amax(ctx, io.in, (long long)B * H * W, cin, io.in_ld, in_slot);
        if (!amax) return DT_ERR_DEVICE;
        w.nt = 2; w.amax = amax;
    }
    w.in = io.in; w.in_bs = io.in_bs; w.in_ld = io.in_ld; w.C = cin; w.v = V;
    w.m = Mp; w.m_ld = N; w.N = N; w.bias = bias; w.bias16 = io.bias16; w.slope = slope;
    w.out = io.out; w.out_bs = io.out_bs; w.out_ld = io.out_ld; w.out2 = io.out2; w.out2_ld = io.out2_ld;
    w.xproj = io.xproj; w.xp_bs = io.xp_bs; w.xp_ld = io.xp_ld;
    w.cstate = io.cstate; w.c_bs = io.c_bs; w.c_ld = io.c_ld;
    {
        ProfScope ps(ctx, "wino_input", 0.0, 4.0 * (double)B * H * W * cin + (u_s3 ? 2.0 * NT : 4.0) * (double)P * mt * cin, tag);
        const int rc = launch_wino_input(ctx->stream, w);
        if (rc) return dt_fail(ctx, launch_code(rc), "%s: Winograd input transform launch failed", tag);
    }
    // direct form of the same layer: in + weights + whatever the output transform writes
    const double df_flops = 2.0 * B * H * W * 9.0 * cin_df * N;
    const double df_bytes = 4.0 * ((double)B * H * W * cin_df + 9.0 * cin_df * N + (io.out ? (double)B * H * W * N : 0.0) +
                                   (io.out2 ? (double)B * H * W * N / 4.0 : 0.0) + (io.cstate ? 4.0 * B * H * W * N / 4.0 : 0.0));
    if (u_s3) {
        GemmS3Args g{};
        g.a = w.v_s3; g.b = u_s3; g.c = Mp; g.c_ps = (long long)mt * N; g.P = P; g.Mt = w.Mt; g.Mp = (int)mp; g.N = N; g.Np = npad;
        g.K = cin; g.ldc = N; g.half = ctx->pol.s3_half;
        if (h2) { g.nt = 2; g.pscale = wts.h2_pscale.get(); g.amax = amax; }
        // flops = EXECUTED 16-bit MFMA work (six partial products per multiply, three in the fp16 form); bytes = V + U (NT 16-bit terms each) + M'
        ProfScope ps(ctx, "conv_gemm_s3", wino_gemm_s3_flops(g), (double)P * (2.0 * NT * mt * cin + 2.0 * NT * (double)cin * N + 4.0 * (double)mt * N), tag);
        prof_count(ctx, h2 ? "s3_form:f16x2" : "s3_form:bf16x3");
        prof_direct_form(ctx, df_flops, df_bytes, DF_S3);
        if (ps.on) prof_count(ctx, wino_gemm_s3_half_chosen(g, 0) ? "s3_tile:128x2" : "s3_tile:256");
        const int rc = launch_wino_gemm_s3(ctx->stream, g, 0);
        if (rc) return dt_fail(ctx, launch_code(rc), "%s: split-bf16 Winograd GEMM launch failed (rc=%d)", tag, rc);
    } else {
        ConvArgs a{};
        a.in = V; a.in_ld = cin; a.in_bs = (long long)mt * cin;
        a.wt = wts.u.get(); a.bias = nullptr;
        a.out = Mp; a.out_ld = N; a.out_bs = (long long)mt * N;
        a.B = 1; a.H = 1; a.W = w.Mt; a.Cin = cin; a.N = N; a.M = w.Mt; a.K = cin;
        a.npad = npad; a.slope = 1.0f;
        a.zbatch = P; a.z_in = (long long)mt * cin; a.z_wt = (long long)npad * cin; a.z_out = (long long)mt * N;
        // flops = executed MFMA work of the P GEMMs (the direct form of the same layer is 9*ts*ts/P times
        // that on whole tiles: 4x for F(4x4,3x3), 2.25x for F(2x2,3x3)); bytes = V + U + M'
        ProfScope ps(ctx, "conv_igemm", 2.0 * P * mt * (double)cin * N, 4.0 * P * ((double)mt * cin + (double)cin * N + (double)mt * N), tag);
        prof_direct_form(ctx, df_flops, df_bytes);
        const int rc = launch_igemm(ctx, a, 1, ORD_LINEAR, EPI_PLAIN, pick_cfg_gemm(w.Mt, N, P));
        if (rc) return dt_fail(ctx, launch_code(rc), "%s: Winograd GEMM launch failed (rc=%d)", tag, rc);
    }
    {
        const double outb = (io.out ? (double)B * H * W * N : 0.0) + (io.out2 ? (double)B * H * W * N / 4.0 : 0.0) +
                            (io.cstate ? 3.0 * B * H * W * N / 4.0 + (double)B * H * W * N : 0.0);
        ProfScope ps(ctx, "wino_output", 0.0, 4.0 * ((double)P * mt * N + outb), tag);
        w.amax_out = io.amax_out;
        if (!wino_output_fills_amax(w, io.cstate != nullptr)) w.amax_out = nullptr;      // (the gates transform cannot; choose_conv never asks it to)
        const int rc = launch_wino_output(ctx->stream, w, io.cstate != nullptr);
        if (rc) return dt_fail(ctx, launch_code(rc), "%s: Winograd output transform launch failed", tag);
    }
    return DT_OK;
}

struct Dest { float *p; int ld; };

// Tile configuration for a plain / pooled 3x3 or 1x1 layer.  The loss of the MFMA kernel scales
// with the bytes staged per MFMA, so the 16-wave 256x256 tile (half the staging of 128x128) is
// ~5 % faster on the 3x3 layers -- when Cout is a multiple of 256 and there are enough tiles that
// its single resident workgroup per CU does not lose more to wave quantisation than it gains.
static int pick_cfg(int M, int cout, int ks)
{
    if (cout <= 64) return CFG_128x64;
    if (ks == 3 && cout % 256 == 0) {
        const long long t256 = (long long)((M + 255) / 256) * (cout / 256);
        const long long t128 = (long long)((M + 127) / 128) * (cout / 128);
        const double e256 = (double)t256 / (double)(((t256 + 255) / 256) * 256);
        const double e128 = (double)t128 / (double)(((t128 + 511) / 512) * 512);
        if (e256 * 1.05 > e128) return CFG_256x256;
    }
    // 1x1 layers over a whole batch (short K, thousands of row tiles): the 256-row tile halves the weight staging per
    // MFMA -- conv_7 2.43 -> 2.33, conv_10/12 2.19/2.14 -> 2.10/2.05, conv_15/17 2.03/2.01 -> 1.97/1.93 ms per 1440
    // frames; 256x256 is worse for N = 512 and unusable for N = 128
    if (ks == 1 && cout >= 128 && (long long)((M + 255) / 256) * ((cout + 127) / 128) >= 4096) return CFG_256x128;
    return CFG_128x128;
}

// A 1x1 layer with enough channels and pixels (conv_7 / 10 / 12 / 15 / 17 at the benched size) runs as ONE split GEMM straight on the
// producing layer's fp32 activation: the kernel splits its A fragments itself (wino_gemm_s3.hip, VF), bias as an extra K stage,
// LeakyReLU in the epilogue.  (Rounds 3-4 had the producer's output transform write pre-split rows for it.)
static bool s3_1x1_eligible(const dt_ctx *ctx, const ConvLayer &L, long long M)
{
    return L.ks == 1 && L.wt_s3 && ctx->pol.s3 != 0 && ctx->pol.s3_1x1 != 0 && L.cin % 32 == 0 && L.cout >= 64 && M < (1ll << 31) - 256 &&
           (ctx->pol.s3 == 2 || (L.cin >= S3_MINK && L.cin >= ctx->pol.s3_1x1_mink && M >= ctx->pol.s3_minrows && M >= ctx->pol.s3_1x1_minrows));
}

// Which kernel form a conv layer's launch takes: choose_conv is the one place that decides it (and choose_wino, above, for the Winograd GEMMs); whoever needs to know
// what a launch WILL take -- conv_1 for conv_2's input slot, the conv_3 + conv_4 fusion -- asks it instead of restating its tests.  Both are pure: no launch, no
// workspace, no tag, no profile entry.
enum { CF_S3_1X1, CF_DIRECT_H2, CF_FUSED4, CF_WINO, CF_SPLITK, CF_IGEMM };
struct ConvChoice {
    int form;                  // split 1x1 GEMM / direct fp16-form 3x3 / fused F(4x4) / Winograd / fp32 MFMA kernel with split-K / fp32 MFMA kernel
    bool h2;                   // CF_S3_1X1: the fp16 form of the split GEMM (CF_WINO: wino.nt says; CF_DIRECT_H2 has no other)
    int cfg, ksplit;           // CF_SPLITK, CF_IGEMM: tile configuration; CF_SPLITK: the split count
    const WinoWeights *wts; WinoChoice wino;      // CF_WINO: L.wino or L.wino_alt, and what its launch takes
    bool publishes;            // the launch's epilogue takes max |x| of what it leaves for the next layer into the layer's output slot
};
static ConvChoice choose_conv(const dt_ctx *ctx, const ConvLayer &L, const float *in, int in_ld, int B, int H, int W, const float *out, int order, int epi, bool has_out2)
{
    ConvChoice c{};
    const bool plain = epi == EPI_PLAIN && order == ORD_LINEAR, pool_even = epi == EPI_POOL && !((H | W) & 1);
    const long long blocks = (long long)B * ((H + 15) / 16) * ((W + 15) / 16) * ((L.cout + 127) / 128);      // workgroups of the direct and the fused kernel
    // (the split 1x1 form reads its A rows with 16-byte DMA pieces: a caller tensor at a 4 / 8 / 12-byte offset takes the fp32 kernel instead of failing)
    if (L.bias_s3 && ctx->s3_ones && plain && !has_out2 && in_ld % 4 == 0 && (reinterpret_cast<uintptr_t>(in) & 15) == 0 &&
        (reinterpret_cast<uintptr_t>(out) & 3) == 0 && s3_1x1_eligible(ctx, L, (long long)B * H * W)) {
        c.form = CF_S3_1X1;
        c.h2 = L.wt_h2 && L.pscale_h2 && L.npad <= 2048 && h2_wanted(ctx);
    }
    // conv_2 / 3 / 5's shapes: the DIRECT convolution in the two-term fp16 form (conv3_h2.hip) once there are enough tiles to fill the chip
    else if (L.w3_h2 && L.pscale_w3 && ctx->pol.c3h2 != 0 && h2_wanted(ctx) && in_ld % 4 == 0 && (reinterpret_cast<uintptr_t>(in) & 15) == 0 && (plain || pool_even) &&
             (ctx->pol.c3h2 == 2 || blocks >= C3H2_MIN_BLOCKS))
        c.form = CF_DIRECT_H2;
    // conv_2 / 3 / 5 (6 / 8)'s shapes: the fused F(4x4,3x3) kernel (V and M' stay on the CU) once there are enough 16x16-pixel
    // blocks to fill the chip several times over; below that the unfused forms win (few, half-empty workgroups)
    else if (L.fused4s && ctx->pol.fused4 != 0 && in_ld % 4 == 0 && (plain || pool_even) &&
             (ctx->pol.fused4 == 2 || (((ctx->pol.fused4 == 1 && L.cin <= 64) || ctx->pol.fused4 == 3) && blocks >= 1024)))
        c.form = CF_FUSED4;
    else if (wino_runs(ctx, L.wino, B, H, W, L.cout) && (plain || epi == EPI_POOL || epi == EPI_POOL_BOTH)) {
        const bool pooled = epi == EPI_POOL || has_out2;
        c.form = CF_WINO; c.wts = &L.wino;
        c.wino = choose_wino(ctx, L.wino, L.cout, B, H, W, pooled, false);
        // F(6x6) or F(4x4) for this launch: with many tiles F(6x6)'s fewer multiplies win; with a few frames the choice
        // is about how the positions x row tiles x column tiles spread over the CUs (small_gemm_cost)
        if (L.wino_alt.u && !ctx->pol.pin) {
            const WinoChoice alt = choose_wino(ctx, L.wino_alt, L.cout, B, H, W, pooled, false);
            const long long t6 = 64ll * ((c.wino.q.Mt + 127) / 128) * ((L.cout + 127) / 128);
            // (the cost model prices the fp32 MFMA kernel's tiles: where the F(6x6) launch takes the split GEMM in the fp16 form -- choose_wino's answer -- F(4x4) on the
            //  fp32 kernel is no alternative: at 20 frames it cost the 13x13 layers 0.10-0.24 ms each against 0.05-0.11 on the split kernel)
            if (c.wino.nt != 2 && t6 <= 4096 && small_gemm_cost(alt.q.Mt, L.cout, 36, nullptr) < small_gemm_cost(c.wino.q.Mt, L.cout, 64, nullptr)) {
                c.wts = &L.wino_alt; c.wino = alt;
            }
        }
    } else {
        // Wave quantisation for small batches (few frames at 13x13 / 26x26): with 512 resident
        // workgroup slots (256 CUs x 2) a layer of a few hundred output tiles leaves the chip
        // partly idle or spills a nearly empty last round.  Split K over grid.y into a slab and
        // combine deterministically; the split count minimises a simple round model
        //   time(s) ~ rounds(tiles*s) / s + 0.003*s,  rounds(n) = full rounds + cost of the partial one
        // (a half-empty round still costs ~0.6 of a full one: single workgroups per CU run faster).
        const int M = B * H * W;
        c.form = CF_IGEMM; c.ksplit = 1;
        c.cfg = pick_cfg(M, L.cout, L.ks);
        if (plain && c.cfg != CFG_128x64) {
            const int tiles = ((M + 127) / 128) * ((L.cout + 127) / 128), nk = L.ks * L.ks * L.cin / 32;
            if (tiles < 2 * 512 && !ctx->pol.pin) {      // (DT_PIN: no split-K -- the split count would depend on the batch)
                int smax = nk / 6;                           // keep >= 6 chunks (192 of K) per split
                if (smax > 32) smax = 32;
                double best = 1e30;
                for (int sp = 1; sp <= (smax < 1 ? 1 : smax); ++sp) {
                    const int n = tiles * sp, full = n / 512, part = n % 512;
                    const double rounds = full + (part == 0 ? 0.0 : (part <= 256 ? 0.6 : 0.6 + 0.4 * (part - 256) / 256.0));
                    const double t = rounds / sp + 0.003 * sp;   // + slab write/read and combine launch per split
                    if (t < best - 1e-9) { best = t; c.ksplit = sp; }
                }
            }
            if (c.ksplit > 1) { c.form = CF_SPLITK; c.cfg = CFG_128x128; }   // the split-K path is built for the 128x128 tile
        }
    }
    // publication: wanted, the layer has an output slot, and this form's epilogue can -- split-K's reduce cannot, the fp32 MFMA kernel for these epilogues
    const bool can = c.form != CF_SPLITK && (c.form != CF_IGEMM || epi == EPI_PLAIN || epi == EPI_POOL || epi == EPI_POOL_BOTH || epi == EPI_S2D);
    c.publishes = h2_wanted(ctx) && amax_out_slot(L) && can;
    return c;
}

// one run_conv call as the function of its form sees it; flops / bytes: the direct form of the layer (3x3 and fp32-kernel forms)
struct ConvCall {
    const ConvLayer &L; const float *in; int in_ld, B, H, W; float *out; int out_ld, order, epi; float slope; float *out2; int out2_ld;
    const char *tag; unsigned *amax_out; int M; double flops, bytes;
};

static int conv_s3_1x1(dt_ctx *ctx, const ConvCall &c, bool h2)
{
    const ConvLayer &L = c.L;
    const long long M = (long long)c.B * c.H * c.W;
    GemmS3Args g{};
    g.a_f32 = c.in; g.a_ld = c.in_ld; g.b = L.wt_s3.get(); g.c = c.out; g.c_ps = 0; g.P = 1; g.Mt = (int)M; g.Mp = (int)((M + 255) / 256 * 256); g.N = L.cout; g.Np = L.npad;
    g.half = ctx->pol.s3_half; g.K = L.cin; g.ldc = c.out_ld; g.ones = reinterpret_cast<const unsigned short *>(ctx->s3_ones.get()); g.bias_s3 = L.bias_s3.get(); g.act = 1; g.slope = c.slope;
    if (h2) {      // the fp16 form: scaled operands (the activation's power of two from its max |x|), the bias added in the epilogue
        g.nt = 2; g.b = L.wt_h2.get(); g.pscale = L.pscale_h2.get(); g.bias = L.bias.get(); g.ones = nullptr; g.bias_s3 = nullptr;
        g.amax = ensure_amax(ctx, c.in, M, L.cin, c.in_ld, amax_in_slot(L));
        if (!g.amax) return DT_ERR_DEVICE;
    }
    g.amax_out = c.amax_out;
    prof_count(ctx, h2 ? "s3_form:f16x2" : "s3_form:bf16x3");
    // bytes = A (fp32) + U (NT 16-bit terms) + out
    ProfScope ps(ctx, "conv_gemm_s3", wino_gemm_s3_flops(g), 4.0 * M * L.cin + (h2 ? 4.0 : 6.0) * (double)L.cin * L.cout + 4.0 * (double)M * L.cout, c.tag);
    prof_direct_form(ctx, 2.0 * M * (double)L.cin * L.cout, 4.0 * ((double)M * L.cin + (double)L.cin * L.cout + (double)M * L.cout), DF_S3);
    const int rc = launch_wino_gemm_s3(ctx->stream, g, 0);
    return rc ? dt_fail(ctx, launch_code(rc), "%s: split-bf16 1x1 GEMM launch failed (rc=%d)", c.tag, rc) : DT_OK;
}
// L4: the 1x1 layer applied behind this one in the same launch (conv3_h2.hip's FUSE instance; c.out takes ITS output), or null
static int conv_direct_h2(dt_ctx *ctx, const ConvCall &c, const ConvLayer *L4 = nullptr)
{
    const ConvLayer &L = c.L;
    Conv3H2Args a{};
    a.in = c.in; a.in_bs = (long long)c.H * c.W * c.in_ld; a.in_ld = c.in_ld; a.B = c.B; a.H = c.H; a.W = c.W; a.Cin = L.cin; a.N = L.cout; a.Np = L.npad;
    a.w = L.w3_h2.get(); a.pscale = L.pscale_w3.get(); a.bias = L.bias.get(); a.slope = c.slope;
    if (L4) { a.w1 = L4->wt_h2.get(); a.pscale1 = L4->pscale_h2.get(); a.bias1 = L4->bias.get(); a.N1 = L4->cout; a.Np1 = L4->npad; a.slope1 = c.slope; }
    if (c.epi == EPI_POOL) { a.out2 = c.out; a.out2_ld = c.out_ld; }
    else { a.out = c.out; a.out_ld = c.out_ld; a.out_bs = (long long)c.H * c.W * c.out_ld; }
    a.zeros = ws_get(ctx, "zeros256", 256, /*zero_on_grow=*/true);
    if (!a.zeros) return DT_ERR_DEVICE;
    a.amax = ensure_amax(ctx, c.in, (long long)c.B * c.H * c.W, L.cin, c.in_ld, amax_in_slot(L));
    if (!a.amax) return DT_ERR_DEVICE;
    a.amax_out = c.amax_out;
    if (L4) prof_count(ctx, "conv_direct_h2:fused_1x1");
    const double M = c.M;
    // executed fp16 MFMA FLOPs (three products per multiply, whole tiles); bytes: the input once per channel tile (+ halo 27 / 41 %) and the output (fused: conv_4's)
    ProfScope ps(ctx, "conv_direct_h2", conv3_h2_flops(a),
                 L4 ? 4.0 * (M * L.cin * 1.41 + M * L4->cout)
                    : 4.0 * ((double)c.B * c.H * c.W * L.cin * (L.cout % 128 ? 1.27 : 1.41) * ((L.cout + 127) / 128) + M * L.cout / (c.epi == EPI_POOL ? 4.0 : 1.0)), c.tag);
    if (L4)      // direct form: both layers
        prof_direct_form(ctx, 2.0 * M * (9.0 * L.cin * L.cout + (double)L4->cin * L4->cout),
                         4.0 * (M * L.cin + 9.0 * L.cin * L.cout + 2.0 * M * L.cout + (double)L4->cin * L4->cout + M * L4->cout), DF_C3H2);
    else prof_direct_form(ctx, c.flops, c.bytes, DF_C3H2);
    const int rc = launch_conv3_h2(ctx->stream, a);
    return rc ? dt_fail(ctx, launch_code(rc), L4 ? "%s: fused direct 3x3 + 1x1 launch failed" : "%s: direct fp16-form 3x3 launch failed", c.tag) : DT_OK;
}
static int conv_fused4(dt_ctx *ctx, const ConvCall &c)
{
    const ConvLayer &L = c.L;
    Wino4FusedArgs f{};
    f.in = c.in; f.in_bs = (long long)c.H * c.W * c.in_ld; f.in_ld = c.in_ld; f.B = c.B; f.H = c.H; f.W = c.W; f.Cin = L.cin; f.N = L.cout;
    f.u = L.fused4s.get(); f.bias = L.bias.get(); f.slope = c.slope;
    if (c.epi == EPI_POOL) { f.out2 = c.out; f.out2_ld = c.out_ld; }
    else { f.out = c.out; f.out_ld = c.out_ld; f.out_bs = (long long)c.H * c.W * c.out_ld; }
    // executed MFMA FLOPs: 36 positions x (whole 4x4 tiles) x Cin x N x 2; bytes: input once per 128 output channels (+ halo 27 %) and the output
    const double tiles = (double)c.B * ((c.H + 3) / 4) * ((c.W + 3) / 4);
    ProfScope ps(ctx, "conv_fused", 2.0 * 36.0 * tiles * L.cin * L.cout,
                 4.0 * ((double)c.B * c.H * c.W * L.cin * 1.27 * ((L.cout + 127) / 128) + (double)c.M * L.cout / (c.epi == EPI_POOL ? 4.0 : 1.0)), c.tag);
    prof_direct_form(ctx, c.flops, c.bytes, DF_FUSED);
    float *zeros = ws_get(ctx, "zeros256", 256, /*zero_on_grow=*/true);
    if (!zeros) return DT_ERR_DEVICE;
    f.amax_out = c.amax_out;
    const int rc = launch_wino4s_fused(ctx->stream, f, zeros);
    return rc ? dt_fail(ctx, launch_code(rc), "%s: fused F(4x4) launch failed", c.tag) : DT_OK;
}
static int conv_wino(dt_ctx *ctx, const ConvCall &c, const WinoWeights &wts, const WinoChoice &wc)
{
    WinoIO io{};
    io.in = c.in; io.in_ld = c.in_ld; io.in_bs = (long long)c.H * c.W * c.in_ld;
    if (c.epi == EPI_POOL) { io.out2 = c.out; io.out2_ld = c.out_ld; }
    else { io.out = c.out; io.out_ld = c.out_ld; io.out_bs = (long long)c.H * c.W * c.out_ld; io.out2 = c.out2; io.out2_ld = c.out2_ld; }
    io.amax_out = c.amax_out;
    return run_wino(ctx, wts, wc, c.L.bias.get(), c.L.cout, c.B, c.H, c.W, io, c.slope, c.tag, 0, amax_in_slot(c.L));
}
// the fp32 MFMA kernel (conv_igemm.hip), whole K per tile or split over ksplit slabs and reduced
static int conv_igemm(dt_ctx *ctx, const ConvCall &c, int cfg, int ksplit)
{
    const ConvLayer &L = c.L;
    ConvArgs a{};
    a.in = c.in; a.in_ld = c.in_ld; a.in_bs = (long long)c.H * c.W * c.in_ld;
    a.wt = L.wt.get(); a.bias = L.bias.get();
    a.out = c.out; a.out_ld = c.out_ld; a.out_bs = (long long)c.H * c.W * c.out_ld;
    a.out2 = c.out2; a.out2_ld = c.out2_ld; a.npad = L.npad; a.slope = c.slope;
    a.B = c.B; a.H = c.H; a.W = c.W; a.Cin = L.cin; a.N = L.cout; a.M = c.M; a.K = L.ks * L.ks * L.cin;
    prof_direct_form(ctx, c.flops, c.bytes);
    if (ksplit > 1) {
        float *slab = ws_get(ctx, "splitk", (size_t)ksplit * a.M * L.cout * sizeof(float));
        if (!slab) return DT_ERR_DEVICE;
        ConvArgs b = a;
        b.out = slab; b.out_ld = L.cout; b.ksplit = ksplit; b.bias = nullptr;
        {
            ProfScope ps(ctx, "conv_igemm", c.flops, c.bytes + 4.0 * ksplit * a.M * (double)L.cout, c.tag);
            const int rc = launch_igemm(ctx, b, L.ks, ORD_LINEAR, EPI_PARTIAL, cfg);
            if (rc) return dt_fail(ctx, launch_code(rc), "conv_%d split-K launch failed (rc=%d)", L.idx, rc);
        }
        ProfScope ps2(ctx, "splitk_reduce", 0.0, 4.0 * (ksplit + 1.0) * a.M * (double)L.cout, c.tag);
        if (launch_splitk_reduce(ctx->stream, slab, ksplit, a.M, L.cout, L.bias.get(), c.slope, c.out, c.out_ld))
            return dt_fail(ctx, DT_ERR_DEVICE, "conv_%d split-K reduce launch failed", L.idx);
        return DT_OK;
    }
    ProfScope ps(ctx, "conv_igemm", c.flops, c.bytes, c.tag);
    a.amax_out = c.amax_out;
    const int rc = launch_igemm(ctx, a, L.ks, c.order, c.epi, cfg);
    return rc ? dt_fail(ctx, launch_code(rc), "conv_%d launch failed (rc=%d)", L.idx, rc) : DT_OK;
}

static int run_conv(dt_ctx *ctx, const ConvLayer &L, const float *in, int in_ld, int B, int H, int W, float *out, int out_ld, int order, int epi, float slope,
                    float *out2 = nullptr, int out2_ld = 0)
{
    const Leaves lv = conv_leaves(epi, out, out_ld, out2, out2_ld, (long long)B * H * W, L.cout);
    amax_forget(ctx, lv);
    const ConvChoice ch = choose_conv(ctx, L, in, in_ld, B, H, W, out, order, epi, out2 != nullptr);
    const int M = B * H * W, K = L.ks * L.ks * L.cin;
    char tag[32];
    snprintf(tag, sizeof(tag), L.idx == 102 ? "tconv_2" : "conv_%d", L.idx);
    const ConvCall c{L, in, in_ld, B, H, W, out, out_ld, order, epi, slope, out2, out2_ld, tag, ch.publishes ? amax_slot(ctx, amax_out_slot(L)) : nullptr, M,
                     2.0 * M * (double)K * L.cout, 4.0 * ((double)M * L.cin + (double)K * L.cout + (double)M * L.cout / (epi == EPI_POOL ? 4.0 : 1.0))};
    int rc = DT_ERR_STATE;
    switch (ch.form) {
    case CF_S3_1X1: rc = conv_s3_1x1(ctx, c, ch.h2); break;
    case CF_DIRECT_H2: rc = conv_direct_h2(ctx, c); break;
    case CF_FUSED4: rc = conv_fused4(ctx, c); break;
    case CF_WINO: rc = conv_wino(ctx, c, *ch.wts, ch.wino); break;
    case CF_SPLITK: case CF_IGEMM: rc = conv_igemm(ctx, c, ch.cfg, ch.ksplit); break;
    }
    if (rc == DT_OK && c.amax_out) amax_note(ctx, lv, amax_out_slot(L));      // the tensor the next layer reads now has its max |x| in the layer's slot
    return rc;
}

// What dt_detector_extract wants out of the graph: the output of layer `idx` in one of the forms the reference's
// layer names denote (KerasYOLO.py:279-400): conv_N = the Conv2D output, norm_N = BatchNormalization output,
// leaky_re_lu_N / conv_feat = after LeakyReLU, max_pooling2d_k = after the pool; lambda_1 = space_to_depth(conv_21
// block), concatenate_1 = [skip, main].
enum { EX_CONV = 0, EX_NORM = 1, EX_ACT = 2, EX_POOL = 3, EX_S2D = 4, EX_CAT = 5 };
struct Extract {
    int idx, kind;
    float *out;      // dense [B][h][w][C]
    bool done = false;
};

// layer `L` on its own, un-fused, into ex.out: pre-activation (slope 1) for conv_N / norm_N, then the BatchNorm
// un-folded for conv_N
static int extract_layer(dt_ctx *ctx, const ConvLayer &L, const float *in, int in_ld, int B, int h, int w, Extract &ex)
{
    if (ex.kind == EX_CONV && L.scale && L.scale_has_zero)
        return dt_fail(ctx, DT_ERR_ARG, "conv_%d: a BatchNorm gamma of 0 was folded into the kernel; the raw Conv2D output cannot be recovered", L.idx);
    int rc = run_conv(ctx, L, in, in_ld, B, h, w, ex.out, L.cout, ORD_LINEAR, EPI_PLAIN, ex.kind == EX_ACT ? LEAKY : 1.0f);
    if (rc) return rc;
    if (ex.kind == EX_CONV && L.scale && launch_unfold_bn(ctx->stream, ex.out, (long long)B * h * w, L.cout, L.scale.get(), L.bias.get()))
        return dt_fail(ctx, DT_ERR_DEVICE, "BatchNorm un-fold launch failed");
    ex.done = true;
    return DT_OK;
}

// conv_3 and the 1x1 conv_4 behind it as ONE launch of conv3_h2.hip (its FUSE instance: the 128-channel tensor between them never exists): where
// conv_3 would take the direct fp16-form kernel anyway (choose_conv), conv_4 is a 128 -> <= 64 channel 1x1 layer with fp16-form weights, and DT_C3FUSE is on
static bool conv34_fusable(const dt_ctx *ctx, const ConvLayer &L3, const ConvLayer &L4, const float *in, int in_ld, int B, int H, int W, const float *out)
{
    return ctx->pol.c3fuse != 0 && L3.ks == 3 && L3.cout == 128 && L4.ks == 1 && L4.cin == 128 && L4.cout <= 64 && L4.wt_h2 && L4.pscale_h2 &&
           choose_conv(ctx, L3, in, in_ld, B, H, W, out, ORD_LINEAR, EPI_PLAIN, false).form == CF_DIRECT_H2;
}
static int run_conv34_fused(dt_ctx *ctx, const ConvLayer &L3, const ConvLayer &L4, const float *in, int in_ld, int B, int H, int W, float *out, int out_ld, float slope)
{
    const Leaves lv = conv_leaves(EPI_PLAIN, out, out_ld, nullptr, 0, (long long)B * H * W, L4.cout);
    amax_forget(ctx, lv);
    char tag[32];
    snprintf(tag, sizeof(tag), "conv_%d", L3.idx);
    const ConvCall c{L3, in, in_ld, B, H, W, out, out_ld, ORD_LINEAR, EPI_PLAIN, slope, nullptr, 0, tag, amax_out_slot(L4) ? amax_slot(ctx, amax_out_slot(L4)) : nullptr, B * H * W, 0.0, 0.0};
    const int rc = conv_direct_h2(ctx, c, &L4);
    if (rc == DT_OK && c.amax_out) amax_note(ctx, lv, amax_out_slot(L4));
    return rc;
}

// conv_2 .. conv_21 on the library-owned buffers (bufA holds conv_1's pooled output).  With `ex` the walk stops at
// the requested layer and writes it to ex->out instead.
static int run_trunk(dt_ctx *ctx, int B, float *bufA, float *bufB, float *skip, float *cat, Extract *ex)
{
    const int H = ctx->image_h, W = ctx->image_w;
    float *cur = bufA, *nxt = bufB;
    int h = H / 2, w = W / 2;
    int rc;
    bool cat20 = false;
    for (int li = 1; li < 20; ++li) {   // conv_2 .. conv_20
        const int idx = TRUNK[li][0], pool = TRUNK[li][4];
        const ConvLayer &L = ctx->layers[idx];
        if (ex && ex->idx == idx && ex->kind <= EX_ACT) return extract_layer(ctx, L, cur, L.cin, B, h, w, *ex);
        if (idx == 3 && TRUNK[li + 1][0] == 4) {
            // conv_3 + conv_4 in one launch.  An extraction of conv_4 / norm_4 asks for conv_4 before its LeakyReLU, which the fused launch never forms: two
            // launches (conv_3's own forms returned above); leaky_re_lu_4 is the launch's output, written straight into the caller's tensor (dense, ld 64)
            const bool ex4 = ex && ex->idx == 4;
            float *out34 = ex4 ? ex->out : nxt;
            if (!(ex4 && ex->kind < EX_ACT) && conv34_fusable(ctx, L, ctx->layers[4], cur, L.cin, B, h, w, out34)) {
                rc = run_conv34_fused(ctx, L, ctx->layers[4], cur, L.cin, B, h, w, out34, ctx->layers[4].cout, LEAKY);
                if (ex4) { ex->done = rc == DT_OK; return rc; }
                if (rc) return rc;
                float *t = cur; cur = nxt; nxt = t;      // conv_4's output is in `nxt`: one swap, conv_4's turn of the walk is skipped
                ++li;
                continue;
            }
        }
        if (idx == 13) {   // skip tapped before the pool (KerasYOLO.py:347)
            rc = run_conv(ctx, L, cur, L.cin, B, h, w, skip, 512, ORD_QUAD, EPI_POOL_BOTH, LEAKY, nxt, 512);
        } else if (idx == 20) {   // writes channels [256,1280) of the concat buffer (KerasYOLO.py:391)
            rc = run_conv(ctx, L, cur, L.cin, B, h, w, cat + 256, 1280, ORD_LINEAR, EPI_PLAIN, LEAKY);
            for (const auto &t : ctx->amax_tag) cat20 |= t.lo == cat + 256 && t.slot == 20;      // conv_20's epilogue measured its 1024 channels into slot 20
        } else if (pool) {
            rc = run_conv(ctx, L, cur, L.cin, B, h, w, nxt, L.cout, ORD_QUAD, EPI_POOL, LEAKY);
        } else {
            rc = run_conv(ctx, L, cur, L.cin, B, h, w, nxt, L.cout, ORD_LINEAR, EPI_PLAIN, LEAKY);
        }
        if (rc) return rc;
        if (pool) { h /= 2; w /= 2; }
        if (ex && ex->idx == idx && ex->kind == EX_POOL) {
            HIP_TRY(ctx, hipMemcpyAsync(ex->out, nxt, (size_t)B * h * w * L.cout * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
            ex->done = true;
            return DT_OK;
        }
        if (ex && ex->idx == 21 && idx == 13 && ex->kind != EX_CAT) break;   // conv_21's block only needs the skip tensor
        float *t = cur; cur = nxt; nxt = t;
    }
    if (ex && ex->idx == 21 && ex->kind <= EX_ACT)
        return extract_layer(ctx, ctx->layers[21], skip, 512, B, H / 16, W / 16, *ex);
    if (ex && ex->idx == 21 && ex->kind == EX_S2D) {
        ex->done = true;
        return run_conv(ctx, ctx->layers[21], skip, 512, B, H / 16, W / 16, ex->out, 256, ORD_QUAD, EPI_S2D, LEAKY);
    }
    // conv_21 on the skip tensor + tf.space_to_depth(2) -> channels [0,256) (KerasYOLO.py:386-391)
    rc = run_conv(ctx, ctx->layers[21], skip, 512, B, H / 16, W / 16, cat, 1280, ORD_QUAD, EPI_S2D, LEAKY);
    if (rc) return rc;
    if (cat20 && h2_wanted(ctx)) {      // ... and the 256 channels conv_21's fp32 kernel wrote are added to the same slot: the concat tensor's max |x| (conv_22 reads it)
        const long long rows = (long long)B * (H / 32) * (W / 32);
        ProfScope ps(ctx, "absmax", 0.0, 4.0 * (double)rows * 256, "cat_skip");
        if (launch_absmax(ctx->stream, cat, rows, 256, 1280, 1, 0, amax_slot(ctx, 20), /*zero=*/false)) return dt_fail(ctx, DT_ERR_DEVICE, "absmax launch failed");
        amax_note(ctx, cat, rows * 1280, 1280, 20);
    }
    if (ex && ex->kind == EX_CAT) {
        HIP_TRY(ctx, hipMemcpyAsync(ex->out, cat, (size_t)B * (H / 32) * (W / 32) * 1280 * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
        ex->done = true;
    }
    return DT_OK;
}

// Runs conv_1 .. conv_23.  feat/netout destinations may alias caller buffers.
static int detect_internal(dt_ctx *ctx, const void *frames, int dtype, int B, Dest feat, Dest netout, bool skip23 = false)
{
    if (!ctx->det_loaded) return dt_fail(ctx, DT_ERR_STATE, "detector weights not loaded");
    if (B <= 0) return dt_fail(ctx, DT_ERR_ARG, "batch must be positive");
    if (dtype != DT_FRAMES_U8 && dtype != DT_FRAMES_F32) return dt_fail(ctx, DT_ERR_ARG, "bad frames dtype");
    const int H = ctx->image_h, W = ctx->image_w;
    if ((long long)B * (H / 2) * (W / 2) >= (1ll << 31)) return dt_fail(ctx, DT_ERR_ARG, "batch too large");
    const size_t per_frame = (size_t)(H / 2) * (W / 2) * 32;   // largest activation (floats)
    float *bufA = ws_get(ctx, "actA", per_frame * B * sizeof(float));
    float *bufB = ws_get(ctx, "actB", per_frame * B * sizeof(float));
    float *skip = ws_get(ctx, "skip", (size_t)B * (H / 16) * (W / 16) * 512 * sizeof(float));
    float *cat = ws_get(ctx, "cat", (size_t)B * (H / 32) * (W / 32) * 1280 * sizeof(float));
    if (!bufA || !bufB || !skip || !cat) return DT_ERR_DEVICE;
    ctx->last_batch = B;
    {   // dt_detector_tap may only hand out 'feat' / 'netout' if THIS forward wrote the library-owned workspaces
        auto owned = [&](const char *name, const float *p) {
            auto it = ctx->ws.find(name);
            return it != ctx->ws.end() && it->second.p == static_cast<const void *>(p);
        };
        ctx->tap_feat = owned("feat", feat.p) && feat.ld == 1024;
        ctx->tap_netout = owned("netout", netout.p) && netout.ld == ctx->cb;
    }

    {   // conv_1 + norm_1 + leaky + pool, with x/255 fused
        const bool c1s3 = ctx->pol.s3 != 0 && ctx->pol.s3_conv1 != 0;
        const double c1_bytes = (double)B * H * W * 3.0 * (dtype == DT_FRAMES_U8 ? 1 : 4) + 4.0 * B * (H / 2) * (W / 2) * 32.0;
        // EXECUTED MFMA FLOPs: K = 27 padded to 32 (bf16: 3 partial products per multiply for uint8 frames, 6 for float32 frames) or to 28 (fp32 MFMA)
        // what the launcher will do with this call: the policy asks for the split form, the launcher may still take the fp32 MFMA kernel (uint8
        // frames at an unaligned address) -- the tag and the executed FLOPs are those of the instance that runs
        const Conv1Plan c1p = plan_conv1(frames, dtype, B, H, W, LEAKY, c1s3 && ctx->conv1_w3.get() && ctx->conv1_w3u8.get(), 0);
        if (c1p.rc) return dt_fail(ctx, DT_ERR_ARG, "conv_1: the launcher refuses B=%d H=%d W=%d (even H and W, at most 65535 frames a call)", B, H, W);
        const bool c1bf = c1p.inst != C1_MFMA_F32;
        const double c1_exec = c1bf ? (c1p.inst == C1_S3_F32 ? 6.0 : 3.0) * 2.0 * B * H * W * 32.0 * 32.0 : 2.0 * B * H * W * 28.0 * 32.0;
        ProfScope ps(ctx, "conv1_direct", c1_exec, c1_bytes, c1bf ? "bf16" : "f32");
        prof_direct_form(ctx, 2.0 * B * H * W * 27.0 * 32.0, c1_bytes, DF_CONV1);
        amax_forget(ctx, bufA, (long long)per_frame * B);
        if (int rcz = amax_begin(ctx)) return rcz;
        // (its epilogue takes max |x| of what it writes: conv_2's direct fp16-form kernel scales its input by it)
        // (conv_1 publishes only where conv_2 will read it: the direct fp16-form kernel -- run_trunk's launch of conv_2, asked for ahead of time)
        const bool c2_direct = choose_conv(ctx, ctx->layers[2], bufA, ctx->layers[2].cin, B, H / 2, W / 2, bufB, ORD_QUAD, EPI_POOL, false).form == CF_DIRECT_H2;
        unsigned *am1 = c1s3 && h2_wanted(ctx) && c2_direct && c1p.fills_amax ? amax_slot(ctx, 1) : nullptr;
        if (launch_conv1_direct(ctx->stream, frames, dtype, B, H, W, ctx->conv1_w.get(), ctx->conv1_b.get(), ctx->lut255.get(), LEAKY,
                                bufA, c1s3 ? ctx->conv1_w3.get() : nullptr, c1s3 ? ctx->conv1_w3u8.get() : nullptr, am1))
            return dt_fail(ctx, DT_ERR_DEVICE, "conv_1 launch failed");
        if (am1) amax_note(ctx, bufA, (long long)B * (H / 2) * (W / 2) * 32, 32, 1);
    }
    const int h = H / 32, w = W / 32;
    int rc = graphed(ctx, "trunk:" + std::to_string(B), [&]() -> int {   // conv_2 .. conv_21: library-owned buffers only
        return run_trunk(ctx, B, bufA, bufB, skip, cat, nullptr);
    }, bufA);
    if (rc) return rc;
    // conv_22 -> 'conv_feat'
    rc = run_conv(ctx, ctx->layers[22], cat, 1280, B, h, w, feat.p, feat.ld, ORD_LINEAR, EPI_PLAIN, LEAKY);
    if (rc) return rc;
    // conv_23 (bias, linear) -- unless nobody reads it: the tracker's merged input projection (build_merged_xproj) carries it in its weights
    if (skip23) { ctx->tap_netout = false; return DT_OK; }
    rc = run_conv(ctx, ctx->layers[23], feat.p, feat.ld, B, h, w, netout.p, netout.ld, ORD_LINEAR, EPI_PLAIN, 1.0f);
    return rc;
}

extern "C" int dt_detect_forward(dt_ctx *ctx, const void *d_frames, int frames_dtype, int batch, float *d_netout,
                                 float *d_feat)
{
    if (!ctx || !d_frames) return dt_fail(ctx, DT_ERR_ARG, "null argument");
    call_begin(ctx, batch);
    const int G2 = (ctx->image_h / 32) * (ctx->image_w / 32);
    Dest feat{d_feat, 1024}, net{d_netout, ctx->cb};
    if (!d_feat) {
        feat.p = ws_get(ctx, "feat", (size_t)batch * G2 * 1024 * sizeof(float));
        if (!feat.p) return DT_ERR_DEVICE;
    }
    if (!d_netout) {
        net.p = ws_get(ctx, "netout", (size_t)batch * G2 * ctx->cb * sizeof(float));
        if (!net.p) return DT_ERR_DEVICE;
    }
    return detect_internal(ctx, d_frames, frames_dtype, batch, feat, net);
}

extern "C" int dt_detector_tap(dt_ctx *ctx, const char *name, int batch, float *d_out)
{
    if (!ctx || !name || !d_out) return dt_fail(ctx, DT_ERR_ARG, "null argument");
    if (batch != ctx->last_batch) return dt_fail(ctx, DT_ERR_STATE, "tap batch %d != last forward batch %d", batch, ctx->last_batch);
    const int H = ctx->image_h, W = ctx->image_w;
    const char *wsname = nullptr;
    size_t n = 0;
    if (!strcmp(name, "act_13")) { wsname = "skip"; n = (size_t)batch * (H / 16) * (W / 16) * 512; }
    else if (!strcmp(name, "conv_feat")) { wsname = "feat"; n = (size_t)batch * (H / 32) * (W / 32) * 1024; }
    else if (!strcmp(name, "conv_23")) { wsname = "netout"; n = (size_t)batch * (H / 32) * (W / 32) * ctx->cb; }
    else return dt_fail(ctx, DT_ERR_ARG, "unknown tap '%s'", name);
    auto it = ctx->ws.find(wsname);
    const bool stale = (!strcmp(wsname, "feat") && !ctx->tap_feat) || (!strcmp(wsname, "netout") && !ctx->tap_netout);
    if (it == ctx->ws.end() || it->second.bytes < n * sizeof(float) || stale)
        return dt_fail(ctx, DT_ERR_STATE, "tap '%s' not materialised by the last forward (it wrote caller-owned outputs; "
                       "call dt_detect_forward with d_netout = d_feat = NULL first)", name);
    HIP_TRY(ctx, hipMemcpyAsync(d_out, it->second.p, n * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
    return DT_OK;
}

// layer name -> (layer index, form, output geometry).  Names are the reference's (KerasYOLO.py:279-400) plus the
// names Keras gives its unnamed layers in a fresh session (leaky_re_lu_N, max_pooling2d_k, lambda_1, concatenate_1).
static bool parse_layer_name(const dt_ctx *ctx, const char *name, int *idx, int *kind, int *oh, int *ow, int *oc)
{
    const int H = ctx->image_h, W = ctx->image_w;
    int n = 0;
    char tail = 0;
    auto geom = [&](int layer, bool pooled) {   // output geometry of conv block `layer` (1..23), before / after its pool
        int div = 1, c = 0;
        for (auto &t : TRUNK) {
            if (t[0] == layer) { c = t[3]; if (pooled) div *= 2; break; }
            if (t[4]) div *= 2;
            if (t[0] == 20) break;
        }
        if (layer == 21) { div = 16; c = 64; }
        if (layer == 22) { div = 32; c = 1024; }
        if (layer == 23) { div = 32; c = ctx->cb; }
        *oh = H / div; *ow = W / div; *oc = c;
    };
    if (sscanf(name, "conv_%d%c", &n, &tail) == 1 && n >= 1 && n <= 23) { *idx = n; *kind = EX_CONV; geom(n, false); return true; }
    if (sscanf(name, "norm_%d%c", &n, &tail) == 1 && n >= 1 && n <= 22) { *idx = n; *kind = EX_NORM; geom(n, false); return true; }
    if ((sscanf(name, "leaky_re_lu_%d%c", &n, &tail) == 1 || sscanf(name, "act_%d%c", &n, &tail) == 1) && n >= 1 && n <= 22) {
        *idx = n; *kind = EX_ACT; geom(n, false); return true;
    }
    if (!strcmp(name, "conv_feat")) { *idx = 22; *kind = EX_ACT; geom(22, false); return true; }
    if (sscanf(name, "max_pooling2d_%d%c", &n, &tail) == 1 && n >= 1 && n <= 5) {
        static const int pooled_after[5] = {1, 2, 5, 8, 13};
        *idx = pooled_after[n - 1]; *kind = EX_POOL; geom(*idx, true); return true;
    }
    if (!strcmp(name, "lambda_1")) { *idx = 21; *kind = EX_S2D; *oh = H / 32; *ow = W / 32; *oc = 256; return true; }
    if (!strcmp(name, "concatenate_1")) { *idx = 21; *kind = EX_CAT; *oh = H / 32; *ow = W / 32; *oc = 1280; return true; }
    if (!strcmp(name, "reshape_1") || !strcmp(name, "lambda_2")) { *idx = 23; *kind = EX_CONV; geom(23, false); return true; }
    return false;
}

extern "C" int dt_detector_extract(dt_ctx *ctx, const void *d_frames, int frames_dtype, int batch, const char *layer,
                                   float *d_out, size_t out_floats, int *shape4)
{
    if (ctx) call_begin(ctx, batch);      // the same kernel forms as dt_detect_forward at this batch
    if (!ctx || !layer) return dt_fail(ctx, DT_ERR_ARG, "null argument");
    if (!ctx->cb) return dt_fail(ctx, DT_ERR_STATE, "dt_detector_config must be called first");
    int idx = 0, kind = 0, oh = 0, ow = 0, oc = 0;
    if (!parse_layer_name(ctx, layer, &idx, &kind, &oh, &ow, &oc)) return dt_fail(ctx, DT_ERR_ARG, "No such layer: %s", layer);
    if (shape4) { shape4[0] = batch; shape4[1] = oh; shape4[2] = ow; shape4[3] = oc; }
    if (!d_out) return DT_OK;   // shape query
    if (!d_frames || batch <= 0) return dt_fail(ctx, DT_ERR_ARG, "bad frames / batch");
    if (!ctx->det_loaded) return dt_fail(ctx, DT_ERR_STATE, "detector weights not loaded");
    if (frames_dtype != DT_FRAMES_U8 && frames_dtype != DT_FRAMES_F32) return dt_fail(ctx, DT_ERR_ARG, "bad frames dtype");
    const size_t need = (size_t)batch * oh * ow * oc;
    if (out_floats < need) return dt_fail(ctx, DT_ERR_ARG, "output buffer holds %zu floats, layer %s needs %zu", out_floats, layer, need);
    const int B = batch, H = ctx->image_h, W = ctx->image_w;
    Extract ex{idx, kind, d_out};
    if (idx == 1 && kind <= EX_ACT) {   // conv_1 un-pooled: as a Cin = 32 layer of the MFMA kernel on zero-padded channels
        float *x32 = ws_get(ctx, "extract_x32", (size_t)B * H * W * 32 * sizeof(float));
        if (!x32) return DT_ERR_DEVICE;
        if (launch_expand_rgb32(ctx->stream, d_frames, frames_dtype, (long long)B * H * W, ctx->lut255.get(), x32))
            return dt_fail(ctx, DT_ERR_DEVICE, "channel expansion launch failed");
        int rc = load_conv_layer(ctx, 0, 3, 32, 32, ctx->conv1_hwio32.data(), ctx->conv1_scale.data(), ctx->conv1_shift.data());
        if (rc) return rc;
        ctx->layers[0].idx = 1;
        return extract_layer(ctx, ctx->layers[0], x32, 32, B, H, W, ex);
    }
    if (idx <= 21 || kind == EX_CAT) {
        const size_t per_frame = (size_t)(H / 2) * (W / 2) * 32;
        float *bufA = ws_get(ctx, "actA", per_frame * B * sizeof(float));
        float *bufB = ws_get(ctx, "actB", per_frame * B * sizeof(float));
        float *skip = ws_get(ctx, "skip", (size_t)B * (H / 16) * (W / 16) * 512 * sizeof(float));
        float *cat = ws_get(ctx, "cat", (size_t)B * (H / 32) * (W / 32) * 1280 * sizeof(float));
        if (!bufA || !bufB || !skip || !cat) return DT_ERR_DEVICE;
        ctx->last_batch = 0;            // the tap workspaces no longer hold a complete forward
        ctx->tap_feat = ctx->tap_netout = false;
        const bool c1s3 = ctx->pol.s3 != 0 && ctx->pol.s3_conv1 != 0;
        if (int rcz = amax_begin(ctx)) return rcz;
        if (launch_conv1_direct(ctx->stream, d_frames, frames_dtype, B, H, W, ctx->conv1_w.get(), ctx->conv1_b.get(), ctx->lut255.get(), LEAKY, bufA,
                                c1s3 ? ctx->conv1_w3.get() : nullptr, c1s3 ? ctx->conv1_w3u8.get() : nullptr))
            return dt_fail(ctx, DT_ERR_DEVICE, "conv_1 launch failed");
        if (idx == 1) {   // max_pooling2d_1
            HIP_TRY(ctx, hipMemcpyAsync(d_out, bufA, need * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
            return DT_OK;
        }
        int rc = run_trunk(ctx, B, bufA, bufB, skip, cat, &ex);
        if (rc) return rc;
        return ex.done ? DT_OK : dt_fail(ctx, DT_ERR_ARG, "layer %s was not reached", layer);
    }
    // conv_22 / conv_23 blocks: a whole forward into the library-owned buffers, then the last layer(s) un-fused
    const int G2 = (H / 32) * (W / 32);
    float *feat = ws_get(ctx, "feat", (size_t)B * G2 * 1024 * sizeof(float));
    float *net = ws_get(ctx, "netout", (size_t)B * G2 * ctx->cb * sizeof(float));
    if (!feat || !net) return DT_ERR_DEVICE;
    int rc = detect_internal(ctx, d_frames, frames_dtype, B, Dest{feat, 1024}, Dest{net, ctx->cb});
    if (rc) return rc;
    if (idx == 23) {
        HIP_TRY(ctx, hipMemcpyAsync(d_out, net, need * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
        return DT_OK;
    }
    float *cat = static_cast<float *>(ctx->ws["cat"].p);
    return extract_layer(ctx, ctx->layers[22], cat, 1280, B, H / 32, W / 32, ex);
}

// ---------------------------------------------------------------------------
// frame ingest
// ---------------------------------------------------------------------------
extern "C" int dt_ingest_resize(dt_ctx *ctx, const uint8_t *d_src, int n, int src_h, int src_w, uint8_t *d_dst,
                                int dst_h, int dst_w)
{
    if (!ctx || !d_src || !d_dst) return dt_fail(ctx, DT_ERR_ARG, "null argument");
    if (n <= 0 || src_h <= 0 || src_w <= 0 || dst_h <= 0 || dst_w <= 0 || n > 65535 || dst_h > 65535)
        return dt_fail(ctx, DT_ERR_ARG, "bad ingest shape");
    int *tabs = reinterpret_cast<int *>(ws_get(ctx, "ingest_tabs", sizeof(int) * 4 * ((size_t)dst_w + dst_h)));
    if (!tabs) return DT_ERR_DEVICE;
    const int key[4] = {src_h, src_w, dst_h, dst_w};
    if (memcmp(key, ctx->ing_key, sizeof(key)) != 0) {
        std::vector<int> h(4 * ((size_t)dst_w + dst_h));
        ingest_tables(src_w, dst_w, h.data());
        ingest_tables(src_h, dst_h, h.data() + 4 * (size_t)dst_w);
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        HIP_TRY(ctx, hipMemcpy(tabs, h.data(), h.size() * sizeof(int), hipMemcpyHostToDevice));
        memcpy(ctx->ing_key, key, sizeof(key));
    }
    ProfScope ps(ctx, "ingest", 0.0, 3.0 * n * ((double)src_h * src_w + (double)dst_h * dst_w));
    if (launch_ingest_resize(ctx->stream, d_src, n, src_h, src_w, d_dst, dst_h, dst_w, tabs, tabs + 4 * (size_t)dst_w))
        return dt_fail(ctx, DT_ERR_DEVICE, "ingest launch failed");
    return DT_OK;
}

// one descriptor of dt_ingest_frames / dt_ingest_views, frame i of the call: DT_OK, or DT_ERR_ARG with the frame named in the message
static int check_frame_desc(dt_ctx *ctx, const dt_frame_desc &f, int i)
{
    if (f.reserved != 0) return dt_fail(ctx, DT_ERR_ARG, "frame %d: reserved must be 0", i);
    if (f.format & ~(DT_PIX_SWAP_RB | DT_PIX_NV12)) return dt_fail(ctx, DT_ERR_ARG, "frame %d: unknown pixel format or flag bits 0x%x", i, (unsigned)f.format);
    const bool nv12 = (f.format & ~DT_PIX_SWAP_RB) == DT_PIX_NV12;
    if (f.height < 1 || f.height > 16384 || f.width < 1 || f.width > 16384)
        return dt_fail(ctx, DT_ERR_ARG, "frame %d: size %dx%d is outside [1, 16384]", i, f.height, f.width);
    if (!f.d_plane0 || (nv12 && !f.d_plane1)) return dt_fail(ctx, DT_ERR_ARG, "frame %d: null plane", i);
    if (nv12 && ((f.height | f.width) & 1)) return dt_fail(ctx, DT_ERR_ARG, "frame %d: NV12 needs an even height and width, got %dx%d", i, f.height, f.width);
    if (f.pitch0 < (nv12 ? f.width : 3 * f.width)) return dt_fail(ctx, DT_ERR_ARG, "frame %d: pitch0 %d is below a row's %d bytes", i, f.pitch0, nv12 ? f.width : 3 * f.width);
    if (nv12 && f.pitch1 < f.width) return dt_fail(ctx, DT_ERR_ARG, "frame %d: pitch1 %d is below a chroma row's %d bytes", i, f.pitch1, f.width);
    return DT_OK;
}

// NV12 / RGB24 frames at per-frame sizes and pitches.  Nothing here depends on an earlier call: no table, no workspace, no key (the
// coefficients are computed in the kernel), so a call never waits for the device and leaves dt_ingest_resize's cached table alone.
extern "C" int dt_ingest_frames(dt_ctx *ctx, const dt_frame_desc *h_desc, int n, uint8_t *d_dst, int dst_h, int dst_w)
{
    if (!ctx || !h_desc || !d_dst) return dt_fail(ctx, DT_ERR_ARG, "null argument");
    if (n <= 0 || dst_h <= 0 || dst_w <= 0 || dst_h > 65535) return dt_fail(ctx, DT_ERR_ARG, "bad ingest shape");
    for (int i = 0; i < n; ++i)
        if (int rc = check_frame_desc(ctx, h_desc[i], i)) return rc;
    for (int base = 0; base < n; base += INGEST_FRAMES_PER_LAUNCH) {
        const int count = n - base < INGEST_FRAMES_PER_LAUNCH ? n - base : INGEST_FRAMES_PER_LAUNCH;
        double bytes = 0.0;      // algorithmic: every source byte once (1.5 per NV12 pixel, 3 per RGB24 pixel) + the frames written
        for (int j = 0; j < count; ++j) {
            const dt_frame_desc &f = h_desc[base + j];
            bytes += ((f.format & ~DT_PIX_SWAP_RB) == DT_PIX_NV12 ? 1.5 : 3.0) * f.height * f.width + 3.0 * dst_h * dst_w;
        }
        ProfScope ps(ctx, "ingest", 0.0, bytes);
        if (launch_ingest_frames(ctx->stream, h_desc, base, count, d_dst, dst_h, dst_w)) return dt_fail(ctx, DT_ERR_DEVICE, "ingest launch failed");
    }
    return DT_OK;
}

// ---- frame views ----
// The two host functions need neither a context nor a device: integer arithmetic in int64, for the affine one double division each.
extern "C" int dt_view_fit(int src_w, int src_h, int out_w, int out_h, int mode, int32_t rect[4])
{
    if (!rect || src_w < 1 || src_h < 1 || out_w < 1 || out_h < 1) return DT_ERR_ARG;
    if (mode == DT_FIT_STRETCH) {
        rect[0] = 0; rect[1] = 0; rect[2] = out_w; rect[3] = out_h;
        return DT_OK;
    }
    if (mode != DT_FIT_LETTERBOX) return DT_ERR_ARG;
    const long long sw = src_w, sh = src_h, ow = out_w, oh = out_h;
    long long w, h;
    if (sw * oh >= sh * ow) {
        w = ow;
        h = (sh * ow + sw / 2) / sw;
        if (h < 1) h = 1;
    } else {
        h = oh;
        w = (sw * oh + sh / 2) / sh;
        if (w < 1) w = 1;
    }
    rect[0] = (int32_t)((ow - w) / 2); rect[1] = (int32_t)((oh - h) / 2); rect[2] = (int32_t)w; rect[3] = (int32_t)h;
    return DT_OK;
}

extern "C" int dt_view_affine(const dt_frame_view *v, int out_w, int out_h, float affine[4])
{
    if (!v || !affine || out_w < 1 || out_h < 1 || v->dst_w < 1 || v->dst_h < 1 || v->frame.width < 1 || v->frame.height < 1) return DT_ERR_ARG;
    const long long dw = v->dst_w, dh = v->dst_h, fw = v->frame.width, fh = v->frame.height;
    affine[0] = (float)((double)((long long)out_w * v->src_w) / (double)(dw * fw));
    affine[1] = (float)((double)((long long)v->src_x * dw - (long long)v->dst_x * v->src_w) / (double)(dw * fw));
    affine[2] = (float)((double)((long long)out_h * v->src_h) / (double)(dh * fh));
    affine[3] = (float)((double)((long long)v->src_y * dh - (long long)v->dst_y * v->src_h) / (double)(dh * fh));
    return DT_OK;
}

// dt_ingest_frames with a crop, a placement and a fill per frame.  As there: no table, no workspace, no key, no wait.
extern "C" int dt_ingest_views(dt_ctx *ctx, const dt_frame_view *h_views, int n, uint8_t *d_dst, int out_h, int out_w)
{
    if (!ctx || !h_views || !d_dst) return dt_fail(ctx, DT_ERR_ARG, "null argument");
    if (n <= 0 || out_h <= 0 || out_w <= 0 || out_h > 65535) return dt_fail(ctx, DT_ERR_ARG, "bad ingest shape");
    for (int i = 0; i < n; ++i) {
        const dt_frame_view &v = h_views[i];
        if (int rc = check_frame_desc(ctx, v.frame, i)) return rc;
        if (v.reserved != 0 || v.reserved0 != 0) return dt_fail(ctx, DT_ERR_ARG, "frame %d: the view's reserved fields must be 0", i);
        // (written as subtractions: x + w could wrap an int32)
        if (v.src_w < 1 || v.src_h < 1 || v.src_x < 0 || v.src_y < 0 || v.src_x > v.frame.width - v.src_w || v.src_y > v.frame.height - v.src_h)
            return dt_fail(ctx, DT_ERR_ARG, "frame %d: source rectangle (%d, %d, %d, %d) is empty or not inside the %dx%d frame", i, v.src_x, v.src_y,
                           v.src_w, v.src_h, v.frame.width, v.frame.height);
        if (v.dst_w < 1 || v.dst_h < 1 || v.dst_x < 0 || v.dst_y < 0 || v.dst_w > out_w || v.dst_h > out_h || v.dst_x > out_w - v.dst_w || v.dst_y > out_h - v.dst_h)
            return dt_fail(ctx, DT_ERR_ARG, "frame %d: destination rectangle (%d, %d, %d, %d) is empty or not inside the %dx%d output", i, v.dst_x,
                           v.dst_y, v.dst_w, v.dst_h, out_w, out_h);
    }
    for (int base = 0; base < n; base += INGEST_VIEWS_PER_LAUNCH) {
        const int count = n - base < INGEST_VIEWS_PER_LAUNCH ? n - base : INGEST_VIEWS_PER_LAUNCH;
        double bytes = 0.0;      // algorithmic: every byte of the source rectangles once (1.5 per NV12 pixel, 3 per RGB24 pixel) + the frames written
        for (int j = 0; j < count; ++j) {
            const dt_frame_view &v = h_views[base + j];
            bytes += ((v.frame.format & ~DT_PIX_SWAP_RB) == DT_PIX_NV12 ? 1.5 : 3.0) * v.src_h * v.src_w + 3.0 * out_h * out_w;
        }
        ProfScope ps(ctx, "ingest", 0.0, bytes);
        if (launch_ingest_views(ctx->stream, h_views, base, count, d_dst, out_h, out_w)) return dt_fail(ctx, DT_ERR_DEVICE, "ingest launch failed");
    }
    return DT_OK;
}

extern "C" int dt_boxes_map(dt_ctx *ctx, float *d_boxes, const int *d_counts, int n, int cap, const float *h_affine)
{
    if (!ctx || !d_boxes || !d_counts || !h_affine) return dt_fail(ctx, DT_ERR_ARG, "null argument");
    if (n <= 0 || cap <= 0) return dt_fail(ctx, DT_ERR_ARG, "bad boxes_map shape");
    for (int i = 0; i < n; ++i)
        for (int k = 0; k < 4; ++k)
            if (!std::isfinite(h_affine[(size_t)i * 4 + k])) return dt_fail(ctx, DT_ERR_ARG, "frame %d: affine element %d is not finite", i, k);
    for (int base = 0; base < n; base += BOXES_MAP_FRAMES_PER_LAUNCH) {
        const int count = n - base < BOXES_MAP_FRAMES_PER_LAUNCH ? n - base : BOXES_MAP_FRAMES_PER_LAUNCH;
        ProfScope ps(ctx, "boxes_map", 0.0, 32.0 * count * cap);
        if (launch_boxes_map(ctx->stream, d_boxes, d_counts, base, count, cap, h_affine)) return dt_fail(ctx, DT_ERR_DEVICE, "boxes_map launch failed");
    }
    return DT_OK;
}

// ---------------------------------------------------------------------------
// decode / iou / associate
// ---------------------------------------------------------------------------
static int decode_common(dt_ctx *ctx, const float *d_netout, int batch, int GH, int GW, int NB, int NC,
                         float obj_threshold, float nms_threshold, const float *d_frame_thr, const float *h_anchors,
                         int cap, float *d_boxes, int *d_counts, float *d_classes, float *d_post)
{
    if (!ctx || !d_netout || !d_boxes || !d_counts || !h_anchors) return dt_fail(ctx, DT_ERR_ARG, "null argument");
    if (batch <= 0 || cap <= 0 || NB <= 0 || NB > 32 || NC <= 0) return dt_fail(ctx, DT_ERR_ARG, "bad decode shape");
    float *anch = ws_get(ctx, "dec_anchors", 64 * sizeof(float));
    if (!anch) return DT_ERR_DEVICE;
    // the caller's host buffer may be a temporary: stage it in the context before the (stream-ordered) upload
    if (memcmp(ctx->dec_anchors_host, h_anchors, sizeof(float) * 2 * NB) != 0 || ctx->dec_anchors_n != 2 * NB) {
        memcpy(ctx->dec_anchors_host, h_anchors, sizeof(float) * 2 * NB);
        ctx->dec_anchors_n = 2 * NB;
        HIP_TRY(ctx, hipMemcpyAsync(anch, ctx->dec_anchors_host, sizeof(float) * 2 * NB, hipMemcpyHostToDevice, ctx->stream));
    }
    const size_t fsz = (size_t)GH * GW * NB * (5 + NC);
    float *post = d_post;
    if (!post) {
        post = ws_get(ctx, "dec_post", (size_t)batch * fsz * sizeof(float));
        if (!post) return DT_ERR_DEVICE;
    }
    float *scratch = nullptr;      // grids above 1920 cells: the kernel's per-candidate arrays live in global memory
    if (const size_t sf = decode_scratch_floats(GH, GW, NB)) {
        scratch = ws_get(ctx, "dec_scratch", (size_t)batch * sf * sizeof(float));
        if (!scratch) return DT_ERR_DEVICE;
    }
    ProfScope ps(ctx, "decode_nms", 0.0, 4.0 * 3.0 * batch * (double)fsz);
    const int rc = launch_decode(ctx->stream, d_netout, (long long)fsz, batch, GH, GW, NB, NC, obj_threshold,
                                 nms_threshold, anch, cap, d_boxes, d_counts, d_classes, post, d_frame_thr, scratch);
    if (rc == 2)
        return dt_fail(ctx, DT_ERR_ARG, "decode: grid %dx%dx%d (limit 8192 cells) / %d classes exceeds the kernel's limits", GH, GW,
                       NB, NC);
    if (rc) return dt_fail(ctx, DT_ERR_DEVICE, "decode launch failed");
    return DT_OK;
}

extern "C" int dt_decode(dt_ctx *ctx, const float *d_netout, int batch, int GH, int GW, int NB, int NC,
                         float obj_threshold, float nms_threshold, const float *h_anchors, int cap, float *d_boxes,
                         int *d_counts, float *d_classes, float *d_post)
{
    return decode_common(ctx, d_netout, batch, GH, GW, NB, NC, obj_threshold, nms_threshold, nullptr, h_anchors, cap,
                         d_boxes, d_counts, d_classes, d_post);
}

extern "C" int dt_decode_per_frame(dt_ctx *ctx, const float *d_netout, int batch, int GH, int GW, int NB, int NC,
                                   const float *d_thresholds, const float *h_anchors, int cap, float *d_boxes,
                                   int *d_counts, float *d_classes, float *d_post)
{
    if (!d_thresholds) return dt_fail(ctx, DT_ERR_ARG, "null thresholds");
    return decode_common(ctx, d_netout, batch, GH, GW, NB, NC, 0.0f, 0.0f, d_thresholds, h_anchors, cap, d_boxes,
                         d_counts, d_classes, d_post);
}

extern "C" int dt_bbox_iou(dt_ctx *ctx, const float *d_pairs, int n, float *d_iou)
{
    if (!ctx || !d_pairs || !d_iou) return dt_fail(ctx, DT_ERR_ARG, "null argument");
    if (launch_bbox_iou(ctx->stream, d_pairs, n, d_iou)) return dt_fail(ctx, DT_ERR_DEVICE, "bbox_iou launch failed");
    return DT_OK;
}

// ---- track identity: the fourteen dt_associate* entries (DESIGN.md "Track identity") ---------------------------------------------------
// One path.  A request is the launch's own argument struct: level = ASSOC_FRAME (associate_kernel, the previous-frame rule) or a level
// of the table kernel.  An entry fills what its level has; associate_entry adds tcap and the carry of a stream call.
static AssocTableArgs assoc_args(int level, const float *d_boxes, const int *d_counts, int T, int cap, float thr, int *d_ids, int *d_nids)
{
    AssocTableArgs a{};
    a.level = level; a.boxes = d_boxes; a.counts = d_counts; a.T = T; a.cap = cap; a.thr = thr; a.ids = d_ids; a.nids = d_nids;
    a.min_hits = 1;
    return a;
}

// the parameters a level has; 0 or the message of the refusal, which names the argument
static const char *assoc_params_refusal(const AssocTableArgs &a, bool stream)
{
    if (a.level >= ASSOC_MEMORY && a.max_age < 0) return "max_age must not be negative";
    if (a.level >= ASSOC_MEMORY && !stream && a.tcap < a.cap) return "tcap must not be below cap";
    if (a.level >= ASSOC_MOTION && !(a.gain >= 0.0f && a.gain <= 1.0f)) return "the motion gain must be in [0, 1]";
    if (a.level < ASSOC_TRACKS) return nullptr;
    if (a.min_hits < 1) return "min_hits must be at least 1";
    const int given = (a.out.tracks != nullptr) + (a.out.tinfo != nullptr) + (a.out.tcounts != nullptr);
    if (given != 0 && given != 3) return "d_tracks, d_tinfo and d_tcounts are given all three or none";
    if (a.assign && a.match != 0 && a.match != DT_MATCH_ANY_LABEL) return "match must be 0 or DT_MATCH_ANY_LABEL: an order means nothing to an assignment";
    if (a.match < 0 || a.match > (DT_MATCH_BEST_FIRST | DT_MATCH_ANY_LABEL)) return "match must be a combination of DT_MATCH_BEST_FIRST and DT_MATCH_ANY_LABEL";
    if (a.scored) {
        if (a.score.at < 0 || a.score.at >= DT_BOX_FLOATS) return "score_at must be in 0..7";
        if (a.score.high != a.score.high || a.score.fresh != a.score.fresh) return "score_high and score_new must not be NaN";
        if (a.score.thr_low != a.score.thr_low) return "the low association threshold must not be NaN";
        if (a.score.max_age_low < -1) return "max_age_low must be at least -1 (-1: no second pass)";
    }
    return nullptr;
}

// the slots' association state as a level's kernel sees it: the arrays of the levels above it stay null
static AssocCarry assoc_carry(StreamTable &S, int level)
{
    AssocCarry c{S.list.get(), S.boxes.get(), S.ids.get(), S.ages.get(), S.meta.get(), S.tcap};
    if (level >= ASSOC_MOTION) { c.vel = S.vel.get(); c.vstamp = S.vstamp.get(); }
    if (level >= ASSOC_TRACKS) { c.hits = S.hits.get(); c.hstamp = S.hstamp.get(); }
    return c;
}

// h_slots: a stream call (clip i continues slot h_slots[i], at the stream table's cap and tcap); null with stream = false: stateless
static int associate_entry(dt_ctx *ctx, AssocTableArgs a, int n, bool stream, const int *h_slots)
{
    static const char *const level_tag[2][4] = {{nullptr, "memory", "motion", "tracks"}, {"stream", "stream_memory", "stream_motion", "stream_tracks"}};
    static const double level_words[4] = {9.0, 10.0, 12.0, 13.0};      // moved per box: the profile's byte estimate
    if (!ctx || !a.boxes || !a.counts || !a.ids || !a.nids) return dt_fail(ctx, DT_ERR_ARG, "null argument");
    if (stream && (n <= 0 || a.T <= 0)) return dt_fail(ctx, DT_ERR_ARG, "n and T must be positive");
    if (const char *why = assoc_params_refusal(a, stream)) return dt_fail(ctx, DT_ERR_ARG, "%s", why);
    if (stream) {
        const int rc = streams_check_list(ctx, h_slots, n);
        if (rc) return rc;
        StreamTable &S = ctx->streams;
        if (a.cap != S.cap) return dt_fail(ctx, DT_ERR_ARG, "cap %d differs from the stream table's %d", a.cap, S.cap);
        a.tcap = S.tcap;
        // refused before the slot list is written, so that an error launches nothing
        if (a.level >= ASSOC_MEMORY && assoc_table_lds_bytes(a.level, a.T, a.cap, a.tcap, assoc_kernel_match(a)) > 160 * 1024)
            return dt_fail(ctx, DT_ERR_ARG, "a track table of %d entries%s%s does not fit the LDS", a.tcap,
                           a.level == ASSOC_MOTION ? " with velocities" : a.level == ASSOC_TRACKS ? " with velocities and hit counts" : "",
                           a.scored ? " and the scored assignment's words per box and per entry" : a.assign ? " and the assignment's words per box and per entry" : (a.match & DT_MATCH_BEST_FIRST) ? " and the best-first order's words per box" : "");
        if (launch_stream_slots(ctx->stream, h_slots, n, S.list.get(), nullptr)) return dt_fail(ctx, DT_ERR_DEVICE, "slot list launch failed");
        a.carry = assoc_carry(S, a.level);
    }
    const double box_bytes = (double)(stream ? a.T + 2 : a.T) * a.cap * level_words[a.level];      // a stream call also reads and leaves the table
    const double row_bytes = a.out.tracks ? (double)a.T * a.tcap * 12.0 : 0.0;
    const char *tag = level_tag[stream][a.level];
    if (a.match) tag = stream ? "stream_tracks_match" : "tracks_match";
    if (a.assign) tag = stream ? "stream_tracks_assign" : "tracks_assign";
    if (a.scored) tag = stream ? "stream_tracks_scored" : "tracks_scored";
    ProfScope ps(ctx, "associate", 0.0, 4.0 * n * (box_bytes + row_bytes), tag);
    int rc;
    if (!stream && a.assign && assoc_table_lds_bytes(a.level, a.T, a.cap, a.tcap, assoc_kernel_match(a)) > 160 * 1024)
        return dt_fail(ctx, DT_ERR_ARG, "tcap: a track table of %d entries with the %sassignment's words per box and per entry does not fit the LDS", a.tcap,
                       a.scored ? "scored " : "");
    if (a.level != ASSOC_FRAME) rc = launch_associate_table(ctx->stream, a, n);
    else if (stream) rc = launch_associate_stream(ctx->stream, a.boxes, a.counts, n, a.T, a.cap, a.thr, a.ids, a.nids, a.carry);
    else rc = launch_associate(ctx->stream, a.boxes, a.counts, n, a.T, a.cap, a.thr, a.ids, a.nids);
    if (rc) return dt_fail(ctx, launch_code(rc), "associate launch failed");
    return DT_OK;
}

extern "C" int dt_associate(dt_ctx *ctx, const float *d_boxes, const int *d_counts, int n_clips, int T, int cap,
                            float assoc_threshold, int *d_ids, int *d_nids)
{
    return associate_entry(ctx, assoc_args(ASSOC_FRAME, d_boxes, d_counts, T, cap, assoc_threshold, d_ids, d_nids), n_clips, false, nullptr);
}

extern "C" int dt_associate_stream(dt_ctx *ctx, const float *d_boxes, const int *d_counts, int n, int T, int cap,
                                   float assoc_threshold, const int *h_slots, int *d_ids, int *d_nids)
{
    return associate_entry(ctx, assoc_args(ASSOC_FRAME, d_boxes, d_counts, T, cap, assoc_threshold, d_ids, d_nids), n, true, h_slots);
}

// the memory and motion entries, stateless (tcap given) and stream (the table's tcap)
static int associate_aged(dt_ctx *ctx, int level, bool stream, const int *h_slots, const float *d_boxes, const int *d_counts, int n, int T, int cap,
                          float thr, int max_age, int tcap, float gain, int *d_ids, int *d_nids, int *d_gaps)
{
    AssocTableArgs a = assoc_args(level, d_boxes, d_counts, T, cap, thr, d_ids, d_nids);
    a.max_age = max_age; a.tcap = tcap; a.gain = gain; a.gaps = d_gaps;
    return associate_entry(ctx, a, n, stream, h_slots);
}

extern "C" int dt_associate_mem(dt_ctx *ctx, const float *d_boxes, const int *d_counts, int n_clips, int T, int cap,
                                float assoc_threshold, int max_age, int tcap, int *d_ids, int *d_nids, int *d_gaps)
{
    return associate_aged(ctx, ASSOC_MEMORY, false, nullptr, d_boxes, d_counts, n_clips, T, cap, assoc_threshold, max_age, tcap, 0.0f, d_ids, d_nids, d_gaps);
}

extern "C" int dt_associate_motion(dt_ctx *ctx, const float *d_boxes, const int *d_counts, int n_clips, int T, int cap,
                                   float assoc_threshold, int max_age, int tcap, float gain, int *d_ids, int *d_nids, int *d_gaps)
{
    return associate_aged(ctx, ASSOC_MOTION, false, nullptr, d_boxes, d_counts, n_clips, T, cap, assoc_threshold, max_age, tcap, gain, d_ids, d_nids, d_gaps);
}

extern "C" int dt_associate_stream_mem(dt_ctx *ctx, const float *d_boxes, const int *d_counts, int n, int T, int cap,
                                       float assoc_threshold, int max_age, const int *h_slots, int *d_ids, int *d_nids, int *d_gaps)
{
    return associate_aged(ctx, ASSOC_MEMORY, true, h_slots, d_boxes, d_counts, n, T, cap, assoc_threshold, max_age, 0, 0.0f, d_ids, d_nids, d_gaps);
}

extern "C" int dt_associate_stream_motion(dt_ctx *ctx, const float *d_boxes, const int *d_counts, int n, int T, int cap,
                                          float assoc_threshold, int max_age, float gain, const int *h_slots, int *d_ids, int *d_nids,
                                          int *d_gaps)
{
    return associate_aged(ctx, ASSOC_MOTION, true, h_slots, d_boxes, d_counts, n, T, cap, assoc_threshold, max_age, 0, gain, d_ids, d_nids, d_gaps);
}

// the tracks entries with the track match policy of the call (DESIGN.md "Track match policy"); match = 0 is dt_associate[_stream]_tracks
// itself.  The policy leaves no trace in a slot: calls with different `match` may follow each other on one slot.
static int associate_tracks(dt_ctx *ctx, bool stream, const int *h_slots, const float *d_boxes, const int *d_counts, int n, int T, int cap, float thr,
                            int max_age, int tcap, float gain, int min_hits, int match, int *d_ids, int *d_nids, int *d_gaps, const TrackReadout &out,
                            bool assign = false, const AssocScore *score = nullptr)
{
    AssocTableArgs a = assoc_args(ASSOC_TRACKS, d_boxes, d_counts, T, cap, thr, d_ids, d_nids);
    a.max_age = max_age; a.tcap = tcap; a.gain = gain; a.min_hits = min_hits; a.match = match; a.gaps = d_gaps; a.out = out; a.assign = assign;
    if (score) { a.scored = true; a.score = *score; }
    return associate_entry(ctx, a, n, stream, h_slots);
}

extern "C" int dt_associate_tracks_match(dt_ctx *ctx, const float *d_boxes, const int *d_counts, int n_clips, int T, int cap,
                                         float assoc_threshold, int max_age, int tcap, float gain, int min_hits, int match, int *d_ids,
                                         int *d_nids, int *d_gaps, int *d_hits, float *d_tracks, int *d_tinfo, int *d_tcounts)
{
    return associate_tracks(ctx, false, nullptr, d_boxes, d_counts, n_clips, T, cap, assoc_threshold, max_age, tcap, gain, min_hits, match, d_ids, d_nids,
                            d_gaps, TrackReadout{d_hits, d_tracks, d_tinfo, d_tcounts});
}

extern "C" int dt_associate_tracks(dt_ctx *ctx, const float *d_boxes, const int *d_counts, int n_clips, int T, int cap,
                                   float assoc_threshold, int max_age, int tcap, float gain, int min_hits, int *d_ids, int *d_nids,
                                   int *d_gaps, int *d_hits, float *d_tracks, int *d_tinfo, int *d_tcounts)
{
    return associate_tracks(ctx, false, nullptr, d_boxes, d_counts, n_clips, T, cap, assoc_threshold, max_age, tcap, gain, min_hits, 0, d_ids, d_nids,
                            d_gaps, TrackReadout{d_hits, d_tracks, d_tinfo, d_tcounts});
}

extern "C" int dt_associate_stream_tracks_match(dt_ctx *ctx, const float *d_boxes, const int *d_counts, int n, int T, int cap,
                                                float assoc_threshold, int max_age, float gain, int min_hits, int match, const int *h_slots,
                                                int *d_ids, int *d_nids, int *d_gaps, int *d_hits, float *d_tracks, int *d_tinfo,
                                                int *d_tcounts)
{
    return associate_tracks(ctx, true, h_slots, d_boxes, d_counts, n, T, cap, assoc_threshold, max_age, 0, gain, min_hits, match, d_ids, d_nids, d_gaps,
                            TrackReadout{d_hits, d_tracks, d_tinfo, d_tcounts});
}

extern "C" int dt_associate_stream_tracks(dt_ctx *ctx, const float *d_boxes, const int *d_counts, int n, int T, int cap,
                                          float assoc_threshold, int max_age, float gain, int min_hits, const int *h_slots, int *d_ids,
                                          int *d_nids, int *d_gaps, int *d_hits, float *d_tracks, int *d_tinfo, int *d_tcounts)
{
    return associate_tracks(ctx, true, h_slots, d_boxes, d_counts, n, T, cap, assoc_threshold, max_age, 0, gain, min_hits, 0, d_ids, d_nids, d_gaps,
                            TrackReadout{d_hits, d_tracks, d_tinfo, d_tcounts});
}

// the tracks entries with the optimal assignment as the match (DESIGN.md "Track assignment"); match: 0 or DT_MATCH_ANY_LABEL
extern "C" int dt_associate_tracks_assign(dt_ctx *ctx, const float *d_boxes, const int *d_counts, int n_clips, int T, int cap,
                                          float assoc_threshold, int max_age, int tcap, float gain, int min_hits, int match, int *d_ids,
                                          int *d_nids, int *d_gaps, int *d_hits, float *d_tracks, int *d_tinfo, int *d_tcounts)
{
    return associate_tracks(ctx, false, nullptr, d_boxes, d_counts, n_clips, T, cap, assoc_threshold, max_age, tcap, gain, min_hits, match, d_ids, d_nids,
                            d_gaps, TrackReadout{d_hits, d_tracks, d_tinfo, d_tcounts}, true);
}

extern "C" int dt_associate_stream_tracks_assign(dt_ctx *ctx, const float *d_boxes, const int *d_counts, int n, int T, int cap,
                                                 float assoc_threshold, int max_age, float gain, int min_hits, int match, const int *h_slots,
                                                 int *d_ids, int *d_nids, int *d_gaps, int *d_hits, float *d_tracks, int *d_tinfo,
                                                 int *d_tcounts)
{
    return associate_tracks(ctx, true, h_slots, d_boxes, d_counts, n, T, cap, assoc_threshold, max_age, 0, gain, min_hits, match, d_ids, d_nids, d_gaps,
                            TrackReadout{d_hits, d_tracks, d_tinfo, d_tcounts}, true);
}

// the assignment entries in two passes by detection score (DESIGN.md "Track scores"); match: 0 or DT_MATCH_ANY_LABEL
extern "C" int dt_associate_tracks_scored(dt_ctx *ctx, const float *d_boxes, const int *d_counts, int n_clips, int T, int cap,
                                          float assoc_threshold, int max_age, int tcap, float gain, int min_hits, int match, int score_at,
                                          float score_high, float score_new, float assoc_threshold_low, int max_age_low, int *d_ids,
                                          int *d_nids, int *d_gaps, int *d_hits, float *d_tracks, int *d_tinfo, int *d_tcounts)
{
    const AssocScore score{score_at, score_high, score_new, assoc_threshold_low, max_age_low};
    return associate_tracks(ctx, false, nullptr, d_boxes, d_counts, n_clips, T, cap, assoc_threshold, max_age, tcap, gain, min_hits, match, d_ids, d_nids,
                            d_gaps, TrackReadout{d_hits, d_tracks, d_tinfo, d_tcounts}, true, &score);
}

extern "C" int dt_associate_stream_tracks_scored(dt_ctx *ctx, const float *d_boxes, const int *d_counts, int n, int T, int cap, float thr,
                                                 int max_age, float gain, int min_hits, int match, int score_at, float score_high,
                                                 float score_new, float thr_low, int max_age_low, const int *h_slots, int *d_ids, int *d_nids,
                                                 int *d_gaps, int *d_hits, float *d_tracks, int *d_tinfo, int *d_tcounts)
{
    const AssocScore score{score_at, score_high, score_new, thr_low, max_age_low};
    return associate_tracks(ctx, true, h_slots, d_boxes, d_counts, n, T, cap, thr, max_age, 0, gain, min_hits, match, d_ids, d_nids, d_gaps,
                            TrackReadout{d_hits, d_tracks, d_tinfo, d_tcounts}, true, &score);
}

// track scoring (DESIGN.md "Track scoring"): CLEAR-MOT counts of hypotheses against ground-truth tracks; the caller owns the state
extern "C" int dt_track_score(dt_ctx *ctx, const float *d_gt_boxes, const int *d_gt_counts, const int *d_gt_ids, int gcap,
                              const float *d_hyp_boxes, const int *d_hyp_counts, const int *d_hyp_ids, int hcap, int id_stride, int hyp_label_at,
                              int n_clips, int T, float iou_threshold, int flags, int ocap, int *d_totals, int *d_objs, int *d_nobjs,
                              int *d_fcounts, int *d_match, float *d_miou)
{
    if (!ctx || !d_gt_boxes || !d_gt_counts || !d_gt_ids || !d_hyp_boxes || !d_hyp_counts || !d_hyp_ids || !d_totals || !d_objs || !d_nobjs)
        return dt_fail(ctx, DT_ERR_ARG, "null argument");
    if (n_clips < 0 || T <= 0 || gcap <= 0 || hcap <= 0 || ocap <= 0) return dt_fail(ctx, DT_ERR_ARG, "n_clips must not be negative; T, gcap, hcap and ocap must be positive");
    if (id_stride < 1) return dt_fail(ctx, DT_ERR_ARG, "id_stride must be at least 1");
    if (hyp_label_at < 0 || hyp_label_at > 7) return dt_fail(ctx, DT_ERR_ARG, "hyp_label_at must be in 0..7");
    if (flags & ~(DT_SCORE_ANY_LABEL | DT_SCORE_RESUME)) return dt_fail(ctx, DT_ERR_ARG, "flags must be a combination of DT_SCORE_ANY_LABEL and DT_SCORE_RESUME");
    if ((d_match != nullptr) != (d_miou != nullptr)) return dt_fail(ctx, DT_ERR_ARG, "d_match and d_miou are given both or neither");
    if (!(iou_threshold > 0.0f && iou_threshold <= 1.0f)) return dt_fail(ctx, DT_ERR_ARG, "the IoU threshold must be in (0, 1]");
    if (track_score_lds_bytes(gcap, hcap, ocap) > (size_t)160 * 1024)
        return dt_fail(ctx, DT_ERR_ARG, "8 * ocap + 11 * gcap + 7 * hcap words do not fit the 160 KB of LDS");
    if (n_clips == 0) return DT_OK;
    ProfScope ps(ctx, "associate", 0.0, 4.0 * n_clips * ((double)T * (gcap * 11.0 + hcap * (8.0 + id_stride)) + ocap * 8.0), "score");
    ScoreArgs a{d_gt_boxes, d_gt_counts, d_gt_ids, d_hyp_boxes, d_hyp_counts, d_hyp_ids, gcap, hcap, id_stride, hyp_label_at, T, ocap,
                iou_threshold, d_totals, d_objs, d_nobjs, d_fcounts, d_match, d_miou};
    const int rc = launch_track_score(ctx->stream, a, n_clips, flags);
    if (rc) return dt_fail(ctx, launch_code(rc), "track score launch failed");
    return DT_OK;
}

// identity scoring (DESIGN.md "Identity scoring"): the overlap of ground-truth with hypothesis trajectories; dt_assign_max on it gives IDTP
extern "C" int dt_identity_overlap(dt_ctx *ctx, const float *d_gt_boxes, const int *d_gt_counts, const int *d_gt_ids, int gcap,
                                   const float *d_hyp_boxes, const int *d_hyp_counts, const int *d_hyp_ids, int hcap, int id_stride,
                                   int hyp_label_at, int n_clips, int T, float iou_threshold, int flags, int acap, int bcap, int *d_sizes,
                                   int *d_gt_tab, int *d_hyp_tab, int *d_overlap)
{
    if (!ctx || !d_gt_boxes || !d_gt_counts || !d_gt_ids || !d_hyp_boxes || !d_hyp_counts || !d_hyp_ids || !d_sizes || !d_gt_tab || !d_hyp_tab ||
        !d_overlap)
        return dt_fail(ctx, DT_ERR_ARG, "null argument");
    if (n_clips < 0 || T <= 0 || gcap <= 0 || hcap <= 0 || acap <= 0 || bcap <= 0)
        return dt_fail(ctx, DT_ERR_ARG, "n_clips must not be negative; T, gcap, hcap, acap and bcap must be positive");
    if (id_stride < 1) return dt_fail(ctx, DT_ERR_ARG, "id_stride must be at least 1");
    if (hyp_label_at < 0 || hyp_label_at > 7) return dt_fail(ctx, DT_ERR_ARG, "hyp_label_at must be in 0..7");
    if (flags & ~(DT_SCORE_ANY_LABEL | DT_SCORE_RESUME)) return dt_fail(ctx, DT_ERR_ARG, "flags must be a combination of DT_SCORE_ANY_LABEL and DT_SCORE_RESUME");
    if (!(iou_threshold > 0.0f && iou_threshold <= 1.0f)) return dt_fail(ctx, DT_ERR_ARG, "the IoU threshold must be in (0, 1]");
    if ((long long)n_clips * acap * bcap >= (1ll << 31)) return dt_fail(ctx, DT_ERR_ARG, "n_clips * acap * bcap must be below 2^31");
    if (identity_overlap_lds_bytes(gcap, hcap, acap, bcap) > (size_t)160 * 1024)
        return dt_fail(ctx, DT_ERR_ARG, "2 * acap + 2 * bcap + 7 * gcap + 7 * hcap words do not fit the 160 KB of LDS");
    if (n_clips == 0) return DT_OK;
    ProfScope ps(ctx, "associate", 0.0, 4.0 * n_clips * ((double)T * (gcap * 6.0 + hcap * (6.0 + id_stride)) + (acap + bcap) * 2.0 + (double)acap * bcap),
                 "identity_overlap");
    IdentArgs a{d_gt_boxes, d_gt_counts, d_gt_ids, d_hyp_boxes, d_hyp_counts, d_hyp_ids, gcap, hcap, id_stride, hyp_label_at, T, acap, bcap,
                iou_threshold, d_sizes, d_gt_tab, d_hyp_tab, d_overlap};
    if (launch_identity_overlap(ctx->stream, a, n_clips, flags)) return dt_fail(ctx, DT_ERR_DEVICE, "identity overlap launch failed");
    return DT_OK;
}

extern "C" int dt_assign_max(dt_ctx *ctx, const int *d_w, int rcap, int ccap, const int *d_dims, int stride, int rows_at, int cols_at, int n,
                             int *d_row_to_col, int *d_col_to_row, int64_t *d_total)
{
    if (!ctx || !d_w || !d_dims || !d_row_to_col || !d_col_to_row || !d_total) return dt_fail(ctx, DT_ERR_ARG, "null argument");
    if (n < 0 || rcap <= 0 || ccap <= 0) return dt_fail(ctx, DT_ERR_ARG, "n must not be negative; rcap and ccap must be positive");
    if (rows_at < 0 || rows_at >= stride || cols_at < 0 || cols_at >= stride) return dt_fail(ctx, DT_ERR_ARG, "rows_at and cols_at must lie inside the stride");
    if ((long long)n * rcap * ccap >= (1ll << 31)) return dt_fail(ctx, DT_ERR_ARG, "n * rcap * ccap must be below 2^31");
    if (assign_max_lds_bytes(rcap, ccap) > (size_t)160 * 1024)
        return dt_fail(ctx, DT_ERR_ARG, "6 * (max(rcap, ccap) + 1) words do not fit the 160 KB of LDS");
    if (n == 0) return DT_OK;
    ProfScope ps(ctx, "associate", 0.0, 4.0 * n * ((double)rcap * ccap + rcap + ccap + 2.0), "assign_max");
    AssignArgs a{d_w, d_dims, rcap, ccap, stride, rows_at, cols_at, d_row_to_col, d_col_to_row, reinterpret_cast<long long *>(d_total)};
    if (launch_assign_max(ctx->stream, a, n)) return dt_fail(ctx, DT_ERR_DEVICE, "assign max launch failed");
    return DT_OK;
}

// HOTA scoring (DESIGN.md "HOTA scoring"): the alignment of a clip's trajectories, every frame's weights for dt_assign_max, and the
// matched pairs counted per IoU level.  The first two share the checks of their input arguments.
static const char *hota_input_args(const void *gt_boxes, const void *gt_counts, const void *gt_ids, int gcap, const void *hyp_boxes,
                                   const void *hyp_counts, const void *hyp_ids, int hcap, int id_stride, int hyp_label_at, int n_clips, int T,
                                   int acap, int bcap, const void *sizes, const void *gt_tab, const void *hyp_tab, const void *align)
{
    if (!gt_boxes || !gt_counts || !gt_ids || !hyp_boxes || !hyp_counts || !hyp_ids || !sizes || !gt_tab || !hyp_tab || !align) return "null argument";
    if (n_clips < 0 || T <= 0 || gcap <= 0 || hcap <= 0 || acap <= 0 || bcap <= 0)
        return "n_clips must not be negative; T, gcap, hcap, acap and bcap must be positive";
    if (id_stride < 1) return "id_stride must be at least 1";
    if (hyp_label_at < 0 || hyp_label_at > 7) return "hyp_label_at must be in 0..7";
    if ((long long)n_clips * acap * bcap >= (1ll << 31)) return "n_clips * acap * bcap must be below 2^31";
    return nullptr;
}

extern "C" int dt_hota_align(dt_ctx *ctx, const float *d_gt_boxes, const int *d_gt_counts, const int *d_gt_ids, int gcap,
                             const float *d_hyp_boxes, const int *d_hyp_counts, const int *d_hyp_ids, int hcap, int id_stride, int hyp_label_at,
                             int n_clips, int T, int flags, int acap, int bcap, int *d_sizes, int *d_gt_tab, int *d_hyp_tab, int64_t *d_align)
{
    if (!ctx) return DT_ERR_ARG;
    if (const char *why = hota_input_args(d_gt_boxes, d_gt_counts, d_gt_ids, gcap, d_hyp_boxes, d_hyp_counts, d_hyp_ids, hcap, id_stride, hyp_label_at,
                                          n_clips, T, acap, bcap, d_sizes, d_gt_tab, d_hyp_tab, d_align))
        return dt_fail(ctx, DT_ERR_ARG, "%s", why);
    if (flags & ~(DT_SCORE_ANY_LABEL | DT_SCORE_RESUME)) return dt_fail(ctx, DT_ERR_ARG, "flags must be a combination of DT_SCORE_ANY_LABEL and DT_SCORE_RESUME");
    if (hota_align_lds_bytes(gcap, hcap, acap, bcap) > (size_t)160 * 1024)
        return dt_fail(ctx, DT_ERR_ARG, "2 * acap + 2 * bcap + 9 * gcap + 9 * hcap words do not fit the 160 KB of LDS");
    if (n_clips == 0) return DT_OK;
    ProfScope ps(ctx, "score", 0.0, 4.0 * n_clips * ((double)T * (gcap * 6.0 + hcap * (6.0 + id_stride)) + (acap + bcap) * 2.0 + 2.0 * acap * bcap),
                 "hota_align");
    HotaArgs a{d_gt_boxes, d_gt_counts, d_gt_ids, d_hyp_boxes, d_hyp_counts, d_hyp_ids, gcap, hcap, id_stride, hyp_label_at, T, acap, bcap,
               d_sizes, d_gt_tab, d_hyp_tab, reinterpret_cast<long long *>(d_align), nullptr, nullptr, nullptr, nullptr};
    if (launch_hota_align(ctx->stream, a, n_clips, flags)) return dt_fail(ctx, DT_ERR_DEVICE, "hota align launch failed");
    return DT_OK;
}

extern "C" int dt_hota_weights(dt_ctx *ctx, const float *d_gt_boxes, const int *d_gt_counts, const int *d_gt_ids, int gcap,
                               const float *d_hyp_boxes, const int *d_hyp_counts, const int *d_hyp_ids, int hcap, int id_stride, int hyp_label_at,
                               int n_clips, int T, int flags, int acap, int bcap, const int *d_sizes, const int *d_gt_tab,
                               const int *d_hyp_tab, const int64_t *d_align, int *d_w, int *d_dims, int *d_gt_ent, int *d_hyp_ent)
{
    if (!ctx) return DT_ERR_ARG;
    if (const char *why = hota_input_args(d_gt_boxes, d_gt_counts, d_gt_ids, gcap, d_hyp_boxes, d_hyp_counts, d_hyp_ids, hcap, id_stride, hyp_label_at,
                                          n_clips, T, acap, bcap, d_sizes, d_gt_tab, d_hyp_tab, d_align))
        return dt_fail(ctx, DT_ERR_ARG, "%s", why);
    if (!d_w || !d_dims || !d_gt_ent || !d_hyp_ent) return dt_fail(ctx, DT_ERR_ARG, "null argument");
    if (flags & ~DT_SCORE_ANY_LABEL) return dt_fail(ctx, DT_ERR_ARG, "flags must be 0 or DT_SCORE_ANY_LABEL");
    if ((long long)n_clips * T * gcap * hcap >= (1ll << 31)) return dt_fail(ctx, DT_ERR_ARG, "n_clips * T * gcap * hcap must be below 2^31");
    if (hota_weights_lds_bytes(gcap, hcap, acap, bcap) > (size_t)160 * 1024)
        return dt_fail(ctx, DT_ERR_ARG, "2 * acap + 2 * bcap + 7 * gcap + 7 * hcap words do not fit the 160 KB of LDS");
    if (n_clips == 0) return DT_OK;
    ProfScope ps(ctx, "score", 0.0, 4.0 * n_clips * T * ((double)gcap * hcap + gcap * 7.0 + hcap * (7.0 + id_stride) + (acap + bcap) * 2.0 + 2.0), "hota_weights");
    // the kernel only reads the four finished arrays: one argument block serves both kernels
    HotaArgs a{d_gt_boxes, d_gt_counts, d_gt_ids, d_hyp_boxes, d_hyp_counts, d_hyp_ids, gcap, hcap, id_stride, hyp_label_at, T, acap, bcap,
               const_cast<int *>(d_sizes), const_cast<int *>(d_gt_tab), const_cast<int *>(d_hyp_tab),
               reinterpret_cast<long long *>(const_cast<int64_t *>(d_align)), d_w, d_dims, d_gt_ent, d_hyp_ent};
    if (launch_hota_weights(ctx->stream, a, n_clips, flags)) return dt_fail(ctx, DT_ERR_DEVICE, "hota weights launch failed");
    return DT_OK;
}

extern "C" int dt_hota_count(dt_ctx *ctx, const float *d_gt_boxes, int gcap, const float *d_hyp_boxes, int hcap, int n_clips, int T,
                             const int *d_dims, const int *d_gt_ent, const int *d_hyp_ent, const int *d_row_to_col, const float *h_thresholds,
                             int n_thr, int acap, int bcap, int flags, int *d_tp, int64_t *d_loc, int *d_pairs)
{
    if (!ctx) return DT_ERR_ARG;
    if (!d_gt_boxes || !d_hyp_boxes || !d_dims || !d_gt_ent || !d_hyp_ent || !d_row_to_col || !h_thresholds || !d_tp || !d_loc || !d_pairs)
        return dt_fail(ctx, DT_ERR_ARG, "null argument");
    if (n_clips < 0 || T <= 0 || gcap <= 0 || hcap <= 0 || acap <= 0 || bcap <= 0)
        return dt_fail(ctx, DT_ERR_ARG, "n_clips must not be negative; T, gcap, hcap, acap and bcap must be positive");
    if (flags & ~DT_SCORE_RESUME) return dt_fail(ctx, DT_ERR_ARG, "flags must be 0 or DT_SCORE_RESUME");
    if (n_thr < 1 || n_thr > DT_HOTA_MAX_THR) return dt_fail(ctx, DT_ERR_ARG, "n_thr must be in 1..32");
    HotaCountArgs a{d_gt_boxes, d_hyp_boxes, d_dims, d_gt_ent, d_hyp_ent, d_row_to_col, gcap, hcap, T, acap, bcap, n_thr, {}, d_tp,
                    reinterpret_cast<long long *>(d_loc), d_pairs};
    for (int k = 0; k < n_thr; ++k) {
        if (!(h_thresholds[k] > 0.0f && h_thresholds[k] <= 1.0f) || (k > 0 && !(h_thresholds[k] > h_thresholds[k - 1])))
            return dt_fail(ctx, DT_ERR_ARG, "the IoU thresholds must be in (0, 1] and strictly ascending");
        a.thr[k] = h_thresholds[k];
    }
    if ((long long)n_clips * n_thr * acap * bcap >= (1ll << 31)) return dt_fail(ctx, DT_ERR_ARG, "n_clips * n_thr * acap * bcap must be below 2^31");
    if ((long long)n_clips * T * gcap >= (1ll << 31) || (long long)n_clips * T * hcap >= (1ll << 31))
        return dt_fail(ctx, DT_ERR_ARG, "n_clips * T * gcap and n_clips * T * hcap must be below 2^31");
    if (n_clips == 0) return DT_OK;
    ProfScope ps(ctx, "score", 0.0, 4.0 * n_clips * ((double)T * (gcap * 19.0 + 2.0) + n_thr * (3.0 + (double)acap * bcap)), "hota_count");
    if (launch_hota_count(ctx->stream, a, n_clips, flags)) return dt_fail(ctx, DT_ERR_DEVICE, "hota count launch failed");
    return DT_OK;
}

// detection scoring (DESIGN.md "Detection scoring"): the VOC match per frame, then every detection's position in its class's score order
static const char *detect_score_args(const void *det_boxes, const void *det_counts, int cap, int score_at, const void *gt_boxes,
                                     const void *gt_counts, int gcap, int B, int NC, int n_thr)
{
    if (B < 0 || cap <= 0 || gcap <= 0 || NC <= 0) return "B must not be negative; cap, gcap and NC must be positive";
    if (B > 0 && (!det_boxes || !det_counts || !gt_boxes || !gt_counts)) return "null argument";      // (no frame: the per-frame arrays are not looked at)
    if (n_thr < 1 || n_thr > DT_DETSCORE_MAX_THR) return "n_thr must be in 1..16";
    if (score_at < 0 || score_at > 7) return "score_at must be in 0..7";
    if ((long long)B * cap >= (1ll << 31) || (long long)B * gcap >= (1ll << 31)) return "B * cap and B * gcap must be below 2^31";
    return nullptr;
}

extern "C" int dt_detect_match(dt_ctx *ctx, const float *d_det_boxes, const int *d_det_counts, int cap, int score_at,
                               const float *d_gt_boxes, const int *d_gt_counts, const int *d_gt_flags, int gcap, int B, int NC,
                               const float *h_thresholds, int n_thr, int *d_state, int *d_best, float *d_iou)
{
    if (!ctx) return DT_ERR_ARG;
    if (!h_thresholds || (B > 0 && (!d_state || !d_best || !d_iou))) return dt_fail(ctx, DT_ERR_ARG, "null argument");
    if (const char *why = detect_score_args(d_det_boxes, d_det_counts, cap, score_at, d_gt_boxes, d_gt_counts, gcap, B, NC, n_thr))
        return dt_fail(ctx, DT_ERR_ARG, "%s", why);
    DetMatchArgs a{d_det_boxes, d_det_counts, d_gt_boxes, d_gt_counts, d_gt_flags, cap, gcap, score_at, B, NC, n_thr, {}, d_state, d_best, d_iou};
    for (int k = 0; k < n_thr; ++k) {
        if (!(h_thresholds[k] > 0.0f && h_thresholds[k] <= 1.0f)) return dt_fail(ctx, DT_ERR_ARG, "every IoU threshold must be in (0, 1]");
        a.thr[k] = h_thresholds[k];
    }
    if (detect_match_lds_bytes(cap, gcap) > (size_t)160 * 1024)
        return dt_fail(ctx, DT_ERR_ARG, "3 * cap + 6 * gcap words do not fit the 160 KB of LDS");
    if (B == 0) return DT_OK;
    ProfScope ps(ctx, "score", 0.0, 4.0 * B * (cap * (8.0 + 2.0 + n_thr) + gcap * 9.0), "detect_match");
    if (launch_detect_match(ctx->stream, a)) return dt_fail(ctx, DT_ERR_DEVICE, "detect match launch failed");
    return DT_OK;
}

extern "C" int dt_detect_rank(dt_ctx *ctx, const float *d_det_boxes, const int *d_det_counts, int cap, int score_at, const int *d_state,
                              const float *d_gt_boxes, const int *d_gt_counts, const int *d_gt_flags, int gcap, int B, int NC, int n_thr,
                              int *d_rank, int *d_ctp, int *d_ngt, int *d_ndet, int *d_ntp)
{
    if (!ctx) return DT_ERR_ARG;
    if ((B > 0 && (!d_state || !d_rank || !d_ctp)) || !d_ngt || !d_ndet || !d_ntp) return dt_fail(ctx, DT_ERR_ARG, "null argument");
    if (const char *why = detect_score_args(d_det_boxes, d_det_counts, cap, score_at, d_gt_boxes, d_gt_counts, gcap, B, NC, n_thr))
        return dt_fail(ctx, DT_ERR_ARG, "%s", why);
    DetRankArgs a{d_det_boxes, d_det_counts, d_state, d_gt_boxes, d_gt_counts, d_gt_flags, cap, gcap, score_at, B, NC, n_thr,
                  d_rank, d_ctp, d_ngt, d_ndet, d_ntp, nullptr, nullptr, nullptr, nullptr, nullptr};
    void *ws = ws_get(ctx, "detect_rank", detect_rank_ws_bytes(B, cap));
    if (!ws) return DT_ERR_DEVICE;
    detect_rank_ws_carve(a, ws);
    ProfScope ps(ctx, "score", 0.0, 4.0 * B * (cap * (2.0 + 3.0 * n_thr) + gcap * 2.0), "detect_rank");
    if (launch_detect_rank(ctx->stream, a)) return dt_fail(ctx, DT_ERR_DEVICE, "detect rank launch failed");
    return DT_OK;
}

// ---------------------------------------------------------------------------
// tracker head (ConvLSTM2D + 1x1)
// ---------------------------------------------------------------------------
extern "C" int dt_tracker_load(dt_ctx *ctx, int units, const float *h_kernel, const float *h_recurrent,
                               const float *h_bias, const float *h_out_kernel, const float *h_out_bias)
{
    if (!ctx || !h_kernel || !h_recurrent || !h_bias || !h_out_kernel || !h_out_bias)
        return dt_fail(ctx, DT_ERR_ARG, "null argument");
    if (!ctx->cb) return dt_fail(ctx, DT_ERR_STATE, "dt_detector_config must be called first");
    if (units <= 0 || units % 32) return dt_fail(ctx, DT_ERR_ARG, "units must be a positive multiple of 32");
    const int U = units, Cb = ctx->cb, Csrc = Cb + 1024;
    const int Cx = round_up(1024 + Cb, 32);   // device z layout: [conv_feat 1024 | x_bbox Cb | zero pad]
    std::vector<int> cin_map(Cx, -1), n_map;
    for (int c = 0; c < 1024; ++c) cin_map[c] = Cb + c;          // Keras order: x_bbox first, then x_vis
    for (int c = 0; c < Cb; ++c) cin_map[1024 + c] = c;
    gate_interleave_map(U, n_map);
    std::vector<float> wx((size_t)4 * U * 9 * Cx), wh((size_t)4 * U * 9 * U), bx((size_t)4 * U);
    pack_conv_weights(h_kernel, 3, Csrc, 4 * U, cin_map.data(), Cx, n_map.data(), 4 * U, nullptr, wx.data());
    pack_conv_weights(h_recurrent, 3, U, 4 * U, nullptr, U, n_map.data(), 4 * U, nullptr, wh.data());
    for (int np = 0; np < 4 * U; ++np) bx[np] = h_bias[n_map[np]];
    const int npad = round_up(Cb, 256);
    std::vector<float> wo((size_t)npad * U), bo(npad, 0.0f);
    pack_conv_weights(h_out_kernel, 1, U, Cb, nullptr, U, nullptr, npad, nullptr, wo.data());
    for (int c = 0; c < Cb; ++c) bo[c] = h_out_bias[c];
    (void)hipStreamSynchronize(ctx->stream);      // queued work may still read the weights these replace
    ConvLayer &Lo = ctx->trk_out;      // tconv_2: wt and bias only -- without the 16-bit forms load_conv_layer builds, it stays on the fp32 MFMA kernel
    int rc;
    if ((rc = upload(ctx, ctx->trk_wx, wx))) return rc;
    if ((rc = upload(ctx, ctx->trk_wh, wh))) return rc;
    if ((rc = upload(ctx, ctx->trk_bx, bx))) return rc;
    if ((rc = upload(ctx, Lo.wt, wo))) return rc;
    if ((rc = upload(ctx, Lo.bias, bo))) return rc;
    ctx->trk_wx_wino = WinoWeights();
    ctx->trk_wh_wino = WinoWeights();
    const int ts_x = wino_tile(ctx, false), ts_h = wino_tile(ctx, true);
    if (wino_wanted(ctx, 3, Cx, 4 * U) &&
        (rc = upload_wino(ctx, ctx->trk_wx_wino, ts_x, h_kernel, Csrc, 4 * U, cin_map.data(), Cx, n_map.data(), 4 * U, nullptr, ts_x == 6)))
        return rc;
    if (wino_wanted(ctx, 3, U, 4 * U) &&
        (rc = upload_wino(ctx, ctx->trk_wh_wino, ts_h, h_recurrent, U, 4 * U, nullptr, U, n_map.data(), 4 * U, nullptr, ts_h == 4)))
        return rc;
    ctx->trk_units = U; ctx->trk_cx = Cx;
    Lo.idx = 102; Lo.ks = 1; Lo.cin = U; Lo.cout = Cb; Lo.npad = npad;
    ctx->trk_hkernel.assign(h_kernel, h_kernel + (size_t)9 * Csrc * 4 * U);
    ctx->trk_hbias.assign(h_bias, h_bias + (size_t)4 * U);
    graphs_clear(ctx);
    ctx->trk_loaded = true;
    if (const int rc = streams_fresh(ctx)) return rc;
    return build_merged_xproj(ctx);
}

// does the input projection of F frames take the merged form (conv_23 folded in)?  The same predicate decides whether dt_track_forward
// may skip conv_23 when the caller does not ask for the detector's grid.
static bool xproj_merged(const dt_ctx *ctx, int F, int gh, int gw)
{
    return ctx->pol.trk_merge && ctx->trk_bx16 && wino_runs(ctx, ctx->trk_wxm_wino, F, gh, gw, 4 * ctx->trk_units);      // (a merged set is F(6x6) always)
}

// xproj = conv3x3(z, Wx) + b for all frames; then the sequential recurrence.
//   z != null, xproj_ext == null : both halves, xproj in the library's workspace (dt_track_forward / dt_track_recurrent)
//   z != null, xproj_ext != null, hseq == null : the input projection ONLY, into the caller's buffer (dt_track_detect_xproj:
//       the projection does not depend on the recurrence, so a frame-sharded deployment runs it where the frame is)
//   z == null, xproj_ext != null : the recurrence ONLY, on the caller's stitched projection rows (dt_track_recurrent_xproj)
// carry (dt_track_stream_forward): clip i continues the stream in slot ctx->streams.list[i] (a DEVICE list, filled by the caller of this
// function before it).  CARRY_WARM: h_{-1} and c come from the slots -- gathered into contiguous rows, and t = 0 is a full recurrent step
// in the form steps t >= 1 take; CARRY_FRESH: every slot of the call is fresh, t = 0 stays the gates-only launch.  Both leave
// h_{T-1} and c in the slots.
enum { CARRY_NONE = 0, CARRY_FRESH = 1, CARRY_WARM = 2 };
static int convlstm_sequence(dt_ctx *ctx, const float *z, int Cx, int n_clips, int T, int gh, int gw, int U,
                             const float *wx, const float *bx, const float *wh, float *hseq /*[n_clips][T][GG][U]*/,
                             const WinoWeights &wx_wino, const WinoWeights &wh_wino, float *xproj_ext = nullptr, int carry = CARRY_NONE)
{
    const int GG = gh * gw, F = n_clips * T, N4 = 4 * U;
    float *h0 = carry == CARRY_WARM ? ws_get(ctx, "trk_h0", (size_t)n_clips * GG * U * sizeof(float)) : nullptr;   // h_{-1} [n_clips][GG][U]
    if (carry == CARRY_WARM && !h0) return DT_ERR_DEVICE;
    float *xproj = xproj_ext ? xproj_ext : ws_get(ctx, "trk_xproj", (size_t)F * GG * N4 * sizeof(float));
    float *cst = hseq ? ws_get(ctx, "trk_c", (size_t)n_clips * GG * U * sizeof(float)) : nullptr;
    if (!xproj || (hseq && !cst)) return DT_ERR_DEVICE;
    // hseq, xproj and the cell state are library-owned, z only when it is the 'trk_z' workspace (dt_track_forward).  A
    // captured graph keeps the pointers it was captured with, so the input projection -- the one part that reads z --
    // is inside the replayed graph only for the library-owned z; for a caller's rows (dt_track_recurrent) it runs
    // plainly and the recurrence alone (3 launches per step, library-owned buffers only) replays, under its own key.
    bool z_owned = false;
    {
        auto it = ctx->ws.find("trk_z");
        z_owned = it != ctx->ws.end() && it->second.p == static_cast<const void *>(z);
    }
    const std::string shape = std::to_string(n_clips) + "x" + std::to_string(T) + (carry == CARRY_WARM ? ":warm" : (carry == CARRY_FRESH ? ":fresh" : ""));
    auto input_projection = [&]() -> int {
    if (z_owned && xproj_merged(ctx, F, gh, gw) && &wx_wino == &ctx->trk_wx_wino) {
        // conv_23 folded into the projection (build_merged_xproj): the 1024 conv_feat channels of z only, border-aware bias -- for the library's OWN z
        // rows only (dt_track_forward, dt_track_detect_xproj): a caller's rows (dt_track_recurrent) may carry any x_bbox and get the two-step form
        WinoIO io;
        memset(&io, 0, sizeof(io));
        io.in = z; io.in_ld = Cx; io.in_bs = (long long)GG * Cx;
        io.out = xproj; io.out_ld = N4; io.out_bs = (long long)GG * N4;
        io.bias16 = ctx->trk_bx16.get() + N4;         // corrections of the 16 border cases; row 0 of the table is the interior bias
        prof_count(ctx, "convlstm_xproj:merged_conv23");
        const int rc = run_wino(ctx, ctx->trk_wxm_wino, choose_wino(ctx, ctx->trk_wxm_wino, N4, F, gh, gw, io), ctx->trk_bx16.get(), N4, F, gh, gw, io, 1.0f, "convlstm_xproj", ctx->cb + 1024, AMAX_TRK);
        if (rc) return rc;
    } else if (wino_runs(ctx, wx_wino, F, gh, gw, N4)) {
        WinoIO io;
        memset(&io, 0, sizeof(io));
        io.in = z; io.in_ld = Cx; io.in_bs = (long long)GG * Cx;
        io.out = xproj; io.out_ld = N4; io.out_bs = (long long)GG * N4;
        const int rc = run_wino(ctx, wx_wino, choose_wino(ctx, wx_wino, N4, F, gh, gw, io), bx, N4, F, gh, gw, io, 1.0f, "convlstm_xproj", ctx->cb + 1024, AMAX_TRK);
        if (rc) return rc;
    } else {
        ConvArgs a;
        memset(&a, 0, sizeof(a));
        a.in = z; a.in_ld = Cx; a.in_bs = (long long)GG * Cx;
        a.wt = wx; a.bias = bx;
        a.out = xproj; a.out_ld = N4; a.out_bs = (long long)GG * N4;
        a.B = F; a.H = gh; a.W = gw; a.Cin = Cx; a.N = N4; a.M = F * GG; a.K = 9 * Cx;
        a.slope = 1.0f;
        ProfScope ps(ctx, "conv_igemm", 2.0 * a.M * 9.0 * (ctx->cb + 1024) * N4,
                     4.0 * ((double)a.M * Cx + (double)a.K * N4 + (double)a.M * N4), "convlstm_xproj");
        a.npad = N4;
        prof_direct_form(ctx, 2.0 * a.M * 9.0 * (ctx->cb + 1024) * N4, 4.0 * ((double)a.M * Cx + (double)a.K * N4 + (double)a.M * N4));
        if (launch_igemm(ctx, a, 3, ORD_LINEAR, EPI_PLAIN, pick_cfg(a.M, N4, 3)))
            return dt_fail(ctx, DT_ERR_DEVICE, "ConvLSTM input projection launch failed");
    }
    return DT_OK;
    };
    auto recurrence = [&]() -> int {
    const long long xp_bs = (long long)T * GG * N4, h_bs = (long long)T * GG * U, c_bs = (long long)GG * U;
    auto state_move = [&](int scatter) -> int {
        const StreamTable &S = ctx->streams;
        StateMove m;
        memset(&m, 0, sizeof(m));
        m.slots = S.list.get(); m.tab_h = S.h.get(); m.tab_c = S.c.get(); m.meta = S.meta.get();
        m.h = scatter ? hseq + (long long)(T - 1) * GG * U : h0; m.h_bs = scatter ? h_bs : c_bs;
        m.c = cst; m.c_bs = c_bs;
        m.n = n_clips; m.row = GG * U; m.scatter = scatter; m.T = T;
        ProfScope ps(ctx, "stream_state", 0.0, 16.0 * n_clips * GG * (double)U, scatter ? "scatter" : "gather");
        return launch_stream_state_move(ctx->stream, m) ? dt_fail(ctx, DT_ERR_DEVICE, "stream state move launch failed") : DT_OK;
    };
    if (carry == CARRY_WARM) {
        if (const int rc = state_move(0)) return rc;
    } else {   // t = 0: h_{-1} = c_{-1} = 0
        ProfScope ps(ctx, "convlstm_gates", 0.0, 4.0 * n_clips * GG * (3.0 * U + 2.0 * U));
        if (launch_convlstm_gates_only(ctx->stream, xproj, xp_bs, N4, cst, c_bs, U, hseq, h_bs, U, n_clips, GG, U))
            return dt_fail(ctx, DT_ERR_DEVICE, "ConvLSTM t=0 launch failed");
    }
    for (int t = carry == CARRY_WARM ? 0 : 1; t < T; ++t) {
        const float *hprev = t ? hseq + (long long)(t - 1) * GG * U : h0;      // (t = 0 of a warm call: the gathered rows)
        const long long hprev_bs = t ? h_bs : c_bs;
        if (wino_runs(ctx, wh_wino, n_clips, gh, gw, N4)) {
            WinoIO io;
            memset(&io, 0, sizeof(io));
            io.in = hprev; io.in_ld = U; io.in_bs = hprev_bs;
            io.out = hseq + (long long)t * GG * U; io.out_ld = U; io.out_bs = h_bs;
            io.xproj = xproj + (long long)t * GG * N4; io.xp_ld = N4; io.xp_bs = xp_bs;
            io.cstate = cst; io.c_ld = U; io.c_bs = c_bs;
            // (h_{t-1} = o * tanh(c) lies in (-1, 1): the fp16 form's scale is static, nothing is measured)
            const int rc = run_wino(ctx, wh_wino, choose_wino(ctx, wh_wino, N4, n_clips, gh, gw, io), nullptr, N4, n_clips, gh, gw, io, 1.0f, "convlstm_step", 0, AMAX_ONE);
            if (rc) return rc;
            continue;
        }
        ConvArgs a;
        memset(&a, 0, sizeof(a));
        a.in = hprev; a.in_ld = U; a.in_bs = hprev_bs;
        a.wt = wh; a.bias = nullptr;
        a.out = hseq + (long long)t * GG * U; a.out_ld = U; a.out_bs = h_bs;
        a.xproj = xproj + (long long)t * GG * N4; a.xp_ld = N4; a.xp_bs = xp_bs;
        a.cstate = cst; a.c_ld = U; a.c_bs = c_bs;
        a.B = n_clips; a.H = gh; a.W = gw; a.Cin = U; a.N = N4; a.M = n_clips * GG; a.K = 9 * U;
        a.slope = 1.0f;
        ProfScope ps(ctx, "conv_igemm", 2.0 * a.M * (double)a.K * N4,
                     4.0 * ((double)a.M * U + (double)a.K * N4 + (double)a.M * N4 + 3.0 * a.M * U), "convlstm_step");
        a.npad = N4;
        prof_direct_form(ctx, 2.0 * a.M * (double)a.K * N4, 4.0 * ((double)a.M * U + (double)a.K * N4 + (double)a.M * N4 + 3.0 * a.M * U));
        if (launch_igemm(ctx, a, 3, ORD_LINEAR, EPI_GATES, pick_cfg(a.M, N4, 3)))
            return dt_fail(ctx, DT_ERR_DEVICE, "ConvLSTM step launch failed");
    }
    return carry != CARRY_NONE ? state_move(1) : DT_OK;
    };
    if (xproj_ext) {       // caller-owned projection rows: nothing here may be baked into a replayed graph
        if (z) { const int rc = input_projection(); if (rc || !hseq) return rc; }
        return hseq ? recurrence() : DT_OK;
    }
    if (z_owned)
        return graphed(ctx, "clstm:" + shape, [&]() -> int {
            const int rc = input_projection();
            return rc ? rc : recurrence();
        }, z);
    const int rc = input_projection();
    return rc ? rc : graphed(ctx, "clstm_steps:" + shape, recurrence);
}

// the recurrent head on z [n_clips][T][G*G][Cx] (library- or caller-owned; null: on the caller's projection rows d_xp): ConvLSTM2D over T, then tconv_2
static int track_recurrent_internal(dt_ctx *ctx, const float *z, int n_clips, int T, float *d_trk, int carry = CARRY_NONE, float *d_xp = nullptr)
{
    const int gh = ctx->image_h / 32, gw = ctx->image_w / 32, GG = gh * gw;
    const int F = n_clips * T, U = ctx->trk_units, Cx = ctx->trk_cx, Cb = ctx->cb;
    float *hseq = ws_get(ctx, "trk_h", (size_t)F * GG * U * sizeof(float));
    if (!hseq) return DT_ERR_DEVICE;
    int rc = convlstm_sequence(ctx, z, Cx, n_clips, T, gh, gw, U, ctx->trk_wx.get(), ctx->trk_bx.get(), ctx->trk_wh.get(), hseq, ctx->trk_wx_wino, ctx->trk_wh_wino, d_xp, carry);
    if (rc) return rc;
    float *trk = d_trk;
    if (!trk) {
        trk = ws_get(ctx, "trk_out", (size_t)F * GG * Cb * sizeof(float));
        if (!trk) return DT_ERR_DEVICE;
    }
    // TimeDistributed(Conv2D(Cb,(1,1)))  'tconv_2'  (MultiObjDetTracker.py:182)
    return run_conv(ctx, ctx->trk_out, hseq, U, F, gh, gw, trk, Cb, ORD_LINEAR, EPI_PLAIN, 1.0f);
}

// the detector's grid, columns [1024, 1024 + Cb) of the z rows, into d_det where the caller asks for it
static int copy_det(dt_ctx *ctx, const float *z, long long rows, float *d_det)
{
    if (d_det && launch_copy_cols(ctx->stream, z + 1024, ctx->trk_cx, d_det, ctx->cb, rows, ctx->cb)) return dt_fail(ctx, DT_ERR_DEVICE, "detection copy launch failed");
    return DT_OK;
}

// dt_track_forward, and with a slot list dt_track_stream_forward: the streams carry their ConvLSTM state from call to call in the context's slots
static int track_forward_internal(dt_ctx *ctx, const void *d_frames, int frames_dtype, int n, int T, const int *h_slots, float *d_trk, float *d_det)
{
    StreamTable &S = ctx->streams;
    const int gh = ctx->image_h / 32, gw = ctx->image_w / 32, GG = gh * gw;
    const int F = n * T, Cx = ctx->trk_cx, Cb = ctx->cb;
    int carry = h_slots ? CARRY_FRESH : CARRY_NONE;
    for (int i = 0; h_slots && i < n; ++i)
        if (S.warm[h_slots[i]]) carry = CARRY_WARM;
    float *z = ws_get_padded(ctx, "trk_z", (size_t)F * GG * Cx * sizeof(float), Cx, 1024 + Cb);
    if (!z) return DT_ERR_DEVICE;
    int rc = detect_internal(ctx, d_frames, frames_dtype, F, Dest{z, Cx}, Dest{z + 1024, Cx}, /*skip23=*/!d_det && xproj_merged(ctx, F, gh, gw));
    if (rc) return rc;
    // the slot list reaches the state moves through the library-owned device list: filled here, in stream order and outside the graph
    if (h_slots && launch_stream_slots(ctx->stream, h_slots, n, S.list.get(), nullptr)) return dt_fail(ctx, DT_ERR_DEVICE, "slot list launch failed");
    rc = track_recurrent_internal(ctx, z, n, T, d_trk, carry);
    if (rc) return rc;
    for (int i = 0; h_slots && i < n; ++i) S.warm[h_slots[i]] = 1;
    if (!d_det) return DT_OK;
    ProfScope ps(ctx, "misc", 0.0, 8.0 * F * GG * (double)Cb);
    return copy_det(ctx, z, (long long)F * GG, d_det);
}

extern "C" int dt_track_forward(dt_ctx *ctx, const void *d_frames, int frames_dtype, int n_clips, int T,
                                float *d_trk, float *d_det)
{
    if (ctx) call_begin(ctx, n_clips * T);
    if (!ctx || !d_frames) return dt_fail(ctx, DT_ERR_ARG, "null argument");
    if (!ctx->trk_loaded) return dt_fail(ctx, DT_ERR_STATE, "tracker weights not loaded");
    if (n_clips <= 0 || T <= 0) return dt_fail(ctx, DT_ERR_ARG, "n_clips and T must be positive");
    return track_forward_internal(ctx, d_frames, frames_dtype, n_clips, T, nullptr, d_trk, d_det);
}

extern "C" int dt_track_stream_forward(dt_ctx *ctx, const void *d_frames, int frames_dtype, int n, int T, const int *h_slots,
                                       float *d_trk, float *d_det)
{
    if (ctx) call_begin(ctx, n * T);
    if (!ctx || !d_frames) return dt_fail(ctx, DT_ERR_ARG, "null argument");
    if (!ctx->trk_loaded) return dt_fail(ctx, DT_ERR_STATE, "tracker weights not loaded");
    if (n <= 0 || T <= 0) return dt_fail(ctx, DT_ERR_ARG, "n and T must be positive");
    int rc = streams_check_list(ctx, h_slots, n);
    if (rc) return rc;
    if (ctx->streams.row != (ctx->image_h / 32) * (ctx->image_w / 32) * ctx->trk_units) return dt_fail(ctx, DT_ERR_STATE, "the stream table was opened for another model");
    return track_forward_internal(ctx, d_frames, frames_dtype, n, T, h_slots, d_trk, d_det);
}

// The two halves of dt_track_forward for a FRAME-sharded deployment (BASELINE.json configs[4]):
// every rank runs the detector on its share of the frames and emits their z rows; the rows are exchanged (RCCL
// all-gather, 13*13*1120*4 = 757 KB per frame at 416); the owner of a clip runs the recurrence on the stitched rows.
extern "C" int dt_track_row_width(dt_ctx *ctx)
{
    return (ctx && ctx->trk_loaded) ? ctx->trk_cx : 0;
}

extern "C" int dt_track_detect(dt_ctx *ctx, const void *d_frames, int frames_dtype, int n_frames, float *d_z)
{
    if (ctx) call_begin(ctx, n_frames);
    if (!ctx || !d_frames || !d_z) return dt_fail(ctx, DT_ERR_ARG, "null argument");
    if (!ctx->trk_loaded) return dt_fail(ctx, DT_ERR_STATE, "tracker weights not loaded");
    if (n_frames <= 0) return dt_fail(ctx, DT_ERR_ARG, "n_frames must be positive");
    const int GG = (ctx->image_h / 32) * (ctx->image_w / 32), Cx = ctx->trk_cx, Cb = ctx->cb;
    if (Cx > 1024 + Cb)   // zero the pad columns [1024+Cb, Cx) of the caller's rows (the ConvLSTM kernel reads them)
        HIP_TRY(ctx, hipMemset2DAsync(d_z + 1024 + Cb, (size_t)Cx * sizeof(float), 0, (size_t)(Cx - 1024 - Cb) * sizeof(float),
                                      (size_t)n_frames * GG, ctx->stream));
    return detect_internal(ctx, d_frames, frames_dtype, n_frames, Dest{d_z, Cx}, Dest{d_z + 1024, Cx});
}

extern "C" int dt_track_recurrent(dt_ctx *ctx, const float *d_z, int n_clips, int T, float *d_trk, float *d_det)
{
    if (ctx) call_begin(ctx, n_clips * T);
    if (!ctx || !d_z) return dt_fail(ctx, DT_ERR_ARG, "null argument");
    if (!ctx->trk_loaded) return dt_fail(ctx, DT_ERR_STATE, "tracker weights not loaded");
    if (n_clips <= 0 || T <= 0) return dt_fail(ctx, DT_ERR_ARG, "n_clips and T must be positive");
    const int rc = track_recurrent_internal(ctx, d_z, n_clips, T, d_trk);
    return rc ? rc : copy_det(ctx, d_z, (long long)n_clips * T * (ctx->image_h / 32) * (ctx->image_w / 32), d_det);
}

// The same split one step later in the graph: the ConvLSTM2D INPUT projection W * x_t + b (MultiObjDetTracker.py:176; 55 % of
// the recurrent head's FLOPs) does not depend on the recurrence, so the rank that ran the detector on a frame runs it too and
// the rows that travel are xproj rows [G, G, 4U] (1.38 MB per frame at 416x416); the clip's owner is left with the sequential part only.
extern "C" int dt_track_xproj_width(dt_ctx *ctx)
{
    return (ctx && ctx->trk_loaded) ? 4 * ctx->trk_units : 0;
}

extern "C" int dt_track_detect_xproj(dt_ctx *ctx, const void *d_frames, int frames_dtype, int n_frames, float *d_xp, float *d_det)
{
    if (ctx) call_begin(ctx, n_frames);
    if (!ctx || !d_frames || !d_xp) return dt_fail(ctx, DT_ERR_ARG, "null argument");
    if (!ctx->trk_loaded) return dt_fail(ctx, DT_ERR_STATE, "tracker weights not loaded");
    if (n_frames <= 0) return dt_fail(ctx, DT_ERR_ARG, "n_frames must be positive");
    const int gh = ctx->image_h / 32, gw = ctx->image_w / 32, GG = gh * gw, Cx = ctx->trk_cx;
    float *z = ws_get_padded(ctx, "trk_z", (size_t)n_frames * GG * Cx * sizeof(float), Cx, 1024 + ctx->cb);
    if (!z) return DT_ERR_DEVICE;
    int rc = detect_internal(ctx, d_frames, frames_dtype, n_frames, Dest{z, Cx}, Dest{z + 1024, Cx}, /*skip23=*/!d_det && xproj_merged(ctx, n_frames, gh, gw));
    if (rc) return rc;
    rc = convlstm_sequence(ctx, z, Cx, n_frames, 1, gh, gw, ctx->trk_units, ctx->trk_wx.get(), ctx->trk_bx.get(), ctx->trk_wh.get(), nullptr,
                           ctx->trk_wx_wino, ctx->trk_wh_wino, d_xp);
    return rc ? rc : copy_det(ctx, z, (long long)n_frames * GG, d_det);
}

extern "C" int dt_track_recurrent_xproj(dt_ctx *ctx, const float *d_xp, int n_clips, int T, float *d_trk)
{
    if (ctx) call_begin(ctx, n_clips * T);
    if (!ctx || !d_xp) return dt_fail(ctx, DT_ERR_ARG, "null argument");
    if (!ctx->trk_loaded) return dt_fail(ctx, DT_ERR_STATE, "tracker weights not loaded");
    if (n_clips <= 0 || T <= 0) return dt_fail(ctx, DT_ERR_ARG, "n_clips and T must be positive");
    return track_recurrent_internal(ctx, nullptr, n_clips, T, d_trk, CARRY_NONE, const_cast<float *>(d_xp));
}

// ---------------------------------------------------------------------------
// TinyTracker
// ---------------------------------------------------------------------------
// ---- the tiny trackers' stream slots (TinyStreamTable, dt_internal.h): the per-object LSTM's h / c carried across calls ----
// Every slot fresh again, in stream order (a zero meta row: the slot's rows read as zeros, recurrent.hip).  U: the units of the model the
// slots are to serve.  A table opened under another U is closed -- a guard for the day the step is compiled for another U: today dt_tiny_load
// refuses units != 512 before it touches anything, so no caller can get there.  dt_tiny_load calls this after its one synchronisation and
// BEFORE its first upload: a load that fails half way leaves no warm state over mixed weights.
static int tiny_streams_fresh(dt_ctx *ctx, int U)
{
    TinyStreamTable &S = ctx->tiny_streams;
    if (!S.n_slots) return DT_OK;
    if (S.U != U) {      // only a load gets here: it has synchronised the stream
        graphs_drop(ctx, ":stream");
        S = TinyStreamTable();
        return DT_OK;
    }
    HIP_TRY(ctx, hipMemsetAsync(S.meta.get(), 0, (size_t)S.n_slots * TSM_META * sizeof(int), ctx->stream));
    return DT_OK;
}

// what every tiny stream call checks before it launches anything: an error leaves every slot as it was
static int tiny_stream_check(dt_ctx *ctx, int n, int T, const int *h_slots)
{
    const TinyStreamTable &S = ctx->tiny_streams;
    if (!ctx->tiny_loaded) return dt_fail(ctx, DT_ERR_STATE, "TinyTracker weights not loaded");
    if (!S.n_slots) return dt_fail(ctx, DT_ERR_STATE, "dt_tiny_stream_open must be called first");
    if (n <= 0 || T <= 0) return dt_fail(ctx, DT_ERR_ARG, "n and T must be positive");
    if (!h_slots || n > S.n_slots) return dt_fail(ctx, DT_ERR_ARG, "a stream call names between 1 and n_slots = %d slots", S.n_slots);
    std::vector<char> seen((size_t)S.n_slots, 0);
    for (int i = 0; i < n; ++i) {
        if (h_slots[i] < 0 || h_slots[i] >= S.n_slots) return dt_fail(ctx, DT_ERR_ARG, "slot %d is outside [0, %d)", h_slots[i], S.n_slots);
        if (seen[h_slots[i]]) return dt_fail(ctx, DT_ERR_ARG, "slot %d is named twice in one call", h_slots[i]);
        seen[h_slots[i]] = 1;
    }
    return DT_OK;
}

// the slot list into the table's device list, 64 numbers per launch, outside any graph; reset_meta: the listed rows are zeroed too
static int tiny_stream_list(dt_ctx *ctx, const int *h_slots, int n, int *reset_meta)
{
    TinyStreamTable &S = ctx->tiny_streams;
    for (int base = 0; base < n; base += 64) {
        ProfScope ps(ctx, "stream_state", 0.0, 4.0 * std::min(64, n - base), reset_meta ? "tiny_reset" : "tiny_slots");
        if (launch_stream_slots(ctx->stream, h_slots + base, std::min(64, n - base), S.list.get() + base, reset_meta))
            return dt_fail(ctx, DT_ERR_DEVICE, "slot list launch failed");
    }
    return DT_OK;
}

extern "C" int dt_tiny_stream_open(dt_ctx *ctx, int n_slots)
{
    if (!ctx) return DT_ERR_ARG;
    if (!ctx->tiny_loaded) return dt_fail(ctx, DT_ERR_STATE, "TinyTracker weights not loaded");
    if (n_slots <= 0 || n_slots > (1 << 20)) return dt_fail(ctx, DT_ERR_ARG, "n_slots must be in [1, %d]", 1 << 20);
    const int U = ctx->tiny_U;
    (void)hipStreamSynchronize(ctx->stream);      // queued steps, and replays of the graphs dropped next, may still use the old table
    graphs_drop(ctx, ":stream");      // captured steps hold the old table's pointers
    TinyStreamTable S;
    HIP_TRY(ctx, S.h.alloc((size_t)2 * n_slots * U));
    HIP_TRY(ctx, S.c.alloc((size_t)n_slots * U));
    HIP_TRY(ctx, S.meta.alloc((size_t)n_slots * TSM_META));
    HIP_TRY(ctx, S.list.alloc((size_t)n_slots));
    HIP_TRY(ctx, hipMemsetAsync(S.meta.get(), 0, (size_t)n_slots * TSM_META * sizeof(int), ctx->stream));
    S.n_slots = n_slots; S.U = U;
    ctx->tiny_streams = std::move(S);
    return DT_OK;
}

extern "C" int dt_tiny_stream_reset(dt_ctx *ctx, const int *h_slots, int n)
{
    if (!ctx) return DT_ERR_ARG;
    if (!ctx->tiny_streams.n_slots) return dt_fail(ctx, DT_ERR_STATE, "dt_tiny_stream_open must be called first");
    if (!h_slots) return tiny_streams_fresh(ctx, ctx->tiny_streams.U);
    if (n == 0) return DT_OK;
    const int rc = tiny_stream_check(ctx, n, 1, h_slots);
    return rc ? rc : tiny_stream_list(ctx, h_slots, n, ctx->tiny_streams.meta.get());
}

extern "C" int dt_tiny_load(dt_ctx *ctx, int D, int units, int out_dim, const float *h_kernel,
                            const float *h_recurrent, const float *h_bias, const float *h_dense_kernel,
                            const float *h_dense_bias)
{
    if (!ctx || !h_kernel || !h_recurrent || !h_bias || !h_dense_kernel || !h_dense_bias)
        return dt_fail(ctx, DT_ERR_ARG, "null argument");
    if (units != 512) return dt_fail(ctx, DT_ERR_ARG, "LSTM units must be 512 (config.json:19)");
    if (D < 8 || out_dim < 1) return dt_fail(ctx, DT_ERR_ARG, "bad D / out_dim");
    const int U = units, Dp = round_up(D, 32), N4 = 4 * U;
    // x.W as a 1x1 "convolution": kernel [D,4U] is HWIO with k=1
    std::vector<float> wx((size_t)N4 * Dp), bx(h_bias, h_bias + N4);
    pack_conv_weights(h_kernel, 1, D, N4, nullptr, Dp, nullptr, N4, nullptr, wx.data());
    // recurrent [U,4U] (k, g*U+j) -> [j][g][k]
    std::vector<float> ur((size_t)U * N4);
    for (int j = 0; j < U; ++j)
        for (int g = 0; g < 4; ++g)
            for (int k = 0; k < U; ++k) ur[((size_t)j * 4 + g) * U + k] = h_recurrent[(size_t)k * N4 + g * U + j];
    // Dense head: O <= 8 (TinyTracker, 4) keeps the [U][O] matrix for the wavefront-reduction
    // kernel; wider heads (TinyHeatmapTracker, 32*32) run as a 1x1 MFMA GEMM with a sigmoid epilogue
    const int O = out_dim, Opad = round_up(O, 256);
    std::vector<float> wd, bd;
    if (O <= 8) {
        wd.assign(h_dense_kernel, h_dense_kernel + (size_t)U * O);
        bd.assign(h_dense_bias, h_dense_bias + O);
    } else {
        wd.resize((size_t)Opad * U);
        pack_conv_weights(h_dense_kernel, 1, U, O, nullptr, U, nullptr, Opad, nullptr, wd.data());
        bd.assign(Opad, 0.0f);
        for (int o = 0; o < O; ++o) bd[o] = h_dense_bias[o];
    }
    (void)hipStreamSynchronize(ctx->stream);      // queued work may still read the weights these replace
    int rc;
    if ((rc = tiny_streams_fresh(ctx, U))) return rc;      // state computed under other weights means nothing
    if ((rc = upload(ctx, ctx->tiny_wx, wx))) return rc;
    if ((rc = upload(ctx, ctx->tiny_bx, bx))) return rc;
    if ((rc = upload(ctx, ctx->tiny_ur, ur))) return rc;
    if ((rc = upload(ctx, ctx->tiny_wd, wd))) return rc;
    if ((rc = upload(ctx, ctx->tiny_bd, bd))) return rc;
    ctx->tiny_D = D; ctx->tiny_Dpad = Dp; ctx->tiny_U = U; ctx->tiny_O = O; ctx->tiny_Opad = Opad;
    graphs_clear(ctx);
    ctx->tiny_loaded = true;
    return DT_OK;
}

extern "C" int dt_tiny_features(dt_ctx *ctx, const float *d_feat, const float *d_det, int n_rows, int fh, int fw,
                                int fc, int pool, float *d_x)
{
    if (!ctx || !d_feat || !d_det || !d_x) return dt_fail(ctx, DT_ERR_ARG, "null argument");
    if (!ctx->tiny_loaded) return dt_fail(ctx, DT_ERR_STATE, "TinyTracker weights not loaded");
    const int D = ctx->tiny_D;
    const int fdim = pool == 0 ? fc : (fh / 4) * (fw / 4) * fc;
    const int ddim = D - fdim;   // 4 (TinyTracker box) or heatmap_size^2 (TinyHeatmapTracker.py:31)
    if (ddim < 1) return dt_fail(ctx, DT_ERR_ARG, "pooled feature width %d leaves no room for the detection input (D %d)", fdim, D);
    // GlobalMaxPooling2D / MaxPooling2D(4,4)+Flatten, then concatenate([x, det]) (TinyTracker.py:29-34)
    ProfScope ps(ctx, "pool", 0.0, 4.0 * n_rows * ((double)fh * fw * fc + fdim));
    int rc = pool == 0 ? launch_global_maxpool(ctx->stream, d_feat, n_rows, fh * fw, fc, d_x, D)
                       : launch_maxpool4_flatten(ctx->stream, d_feat, n_rows, fh, fw, fc, d_x, D);
    if (rc) return dt_fail(ctx, launch_code(rc), "pool launch failed");
    if (launch_copy_cols(ctx->stream, d_det, ddim, d_x + fdim, D, n_rows, ddim))
        return dt_fail(ctx, DT_ERR_DEVICE, "det concat launch failed");
    return DT_OK;
}

// dt_tiny_sequence, and with a slot list (checked by the caller: tiny_stream_check) dt_tiny_stream_sequence: sequence i starts from the state
// in slot h_slots[i] of ctx->tiny_streams and leaves its state after frame T - 1 there.  The stream form launches: the slot list (64 numbers per
// launch), x staging, [the projection, T slot-addressed steps, the slots' bookkeeping] as one graphed sequence, the head.
static int tiny_sequence_internal(dt_ctx *ctx, const float *d_x, int n_seq, int T, const int *h_slots, float *d_out)
{
    const int U = ctx->tiny_U, D = ctx->tiny_D, Dp = ctx->tiny_Dpad, N4 = 4 * U;
    const int R = n_seq * T;
    float *x = ws_get_padded(ctx, "tiny_x", (size_t)R * Dp * sizeof(float), Dp, D);
    float *xproj = ws_get(ctx, "tiny_xproj", (size_t)R * N4 * sizeof(float));
    float *hseq = ws_get(ctx, "tiny_h", (size_t)R * U * sizeof(float));
    float *cst = h_slots ? nullptr : ws_get(ctx, "tiny_c", (size_t)n_seq * U * sizeof(float));
    if (!x || !xproj || !hseq || (!h_slots && !cst)) return DT_ERR_DEVICE;
    TinyStreamTable &S = ctx->tiny_streams;
    // the slot list reaches the steps through the library-owned device list: filled here, in stream order and outside the graph
    if (h_slots) { const int rc = tiny_stream_list(ctx, h_slots, n_seq, nullptr); if (rc) return rc; }
    if (launch_copy_cols(ctx->stream, d_x, D, x, Dp, R, D))   // K padded to a multiple of 32 (pad columns stay 0)
        return dt_fail(ctx, DT_ERR_DEVICE, "x staging launch failed");
    // staged x, xproj, h and c are library-owned: the projection and the T launch-bound steps replay as a graph
    int grc = graphed(ctx, "lstm:" + std::to_string(n_seq) + "x" + std::to_string(T) + (h_slots ? ":stream" : ""), [&]() -> int {
    {   // x.W + b for every (sequence, t) at once on the matrix cores
        ConvArgs a;
        memset(&a, 0, sizeof(a));
        a.in = x; a.in_ld = Dp; a.in_bs = Dp;
        a.wt = ctx->tiny_wx.get(); a.bias = ctx->tiny_bx.get();
        a.out = xproj; a.out_ld = N4; a.out_bs = N4;
        a.B = R; a.H = 1; a.W = 1; a.Cin = Dp; a.N = N4; a.M = R; a.K = Dp;
        a.slope = 1.0f;
        ProfScope ps(ctx, "conv_igemm", 2.0 * R * (double)D * N4, 4.0 * ((double)R * Dp + (double)Dp * N4 + (double)R * N4),
                     "lstm_xproj");
        if (launch_igemm(ctx, a, 1, ORD_LINEAR, EPI_PLAIN, CFG_128x128))
            return dt_fail(ctx, DT_ERR_DEVICE, "LSTM input projection launch failed");
    }
    const long long xp_bs = (long long)T * N4, h_bs = (long long)T * U;
    for (int t = 0; t < T; ++t) {
        ProfScope ps(ctx, "lstm_step", 2.0 * n_seq * (double)U * N4, 4.0 * ((double)U * N4 + n_seq * (6.0 * U + N4)));
        int rc;
        if (h_slots)      // every step in the slot-addressed form: c is the slots' rows, h enters from and leaves to the table
            rc = launch_lstm_step_stream(ctx->stream, xproj + (long long)t * N4, xp_bs, t ? hseq + (long long)(t - 1) * U : nullptr, h_bs,
                                         ctx->tiny_ur.get(), hseq + (long long)t * U, h_bs, n_seq, U,
                                         LstmSlots{S.list.get(), S.meta.get(), S.h.get(), S.c.get(), (long long)S.n_slots * U, t == 0, t == T - 1});
        else if (t == 0)
            rc = launch_lstm_step0(ctx->stream, xproj, xp_bs, cst, hseq, h_bs, n_seq, U);
        else
            rc = launch_lstm_step(ctx->stream, xproj + (long long)t * N4, xp_bs, hseq + (long long)(t - 1) * U, h_bs,
                                  cst, ctx->tiny_ur.get(), hseq + (long long)t * U, h_bs, n_seq, U);
        if (rc) return dt_fail(ctx, DT_ERR_DEVICE, "LSTM step launch failed");
    }
    if (h_slots) {      // the copy the last step wrote becomes current, the frame counters advance (T is part of the graph's key)
        ProfScope ps(ctx, "stream_state", 0.0, 24.0 * n_seq, "tiny_advance");
        if (launch_lstm_stream_advance(ctx->stream, S.list.get(), S.meta.get(), n_seq, T)) return dt_fail(ctx, DT_ERR_DEVICE, "stream bookkeeping launch failed");
    }
    return DT_OK;
    });
    if (grc) return grc;
    const int O = ctx->tiny_O;
    if (O <= 8) {
        ProfScope ps(ctx, "misc", 2.0 * R * U * (double)O, 4.0 * R * (U + (double)O));
        if (launch_dense_sigmoid(ctx->stream, hseq, U, ctx->tiny_wd.get(), ctx->tiny_bd.get(), R, U, O, d_out, O))
            return dt_fail(ctx, DT_ERR_DEVICE, "Dense launch failed");
    } else {   // TimeDistributed(Dense(heatmap_size^2, sigmoid))  (TinyHeatmapTracker.py:43)
        ConvArgs a;
        memset(&a, 0, sizeof(a));
        a.in = hseq; a.in_ld = U; a.in_bs = U;
        a.wt = ctx->tiny_wd.get(); a.bias = ctx->tiny_bd.get();
        a.out = d_out; a.out_ld = O; a.out_bs = O;
        a.B = R; a.H = 1; a.W = 1; a.Cin = U; a.N = O; a.M = R; a.K = U;
        a.slope = 1.0f; a.act = 1;
        ProfScope ps(ctx, "conv_igemm", 2.0 * R * (double)U * O, 4.0 * ((double)R * U + (double)U * O + (double)R * O), "dense_head");
        if (launch_igemm(ctx, a, 1, ORD_LINEAR, EPI_PLAIN, CFG_128x128))
            return dt_fail(ctx, DT_ERR_DEVICE, "Dense head launch failed");
    }
    return DT_OK;
}

extern "C" int dt_tiny_sequence(dt_ctx *ctx, const float *d_x, int n_seq, int T, float *d_out)
{
    if (!ctx || !d_x || !d_out) return dt_fail(ctx, DT_ERR_ARG, "null argument");
    if (!ctx->tiny_loaded) return dt_fail(ctx, DT_ERR_STATE, "TinyTracker weights not loaded");
    if (n_seq <= 0 || T <= 0) return dt_fail(ctx, DT_ERR_ARG, "n_seq and T must be positive");
    return tiny_sequence_internal(ctx, d_x, n_seq, T, nullptr, d_out);
}

extern "C" int dt_tiny_stream_sequence(dt_ctx *ctx, const float *d_x, int n, int T, const int *h_slots, float *d_out)
{
    if (!ctx || !d_x || !d_out) return dt_fail(ctx, DT_ERR_ARG, "null argument");
    const int rc = tiny_stream_check(ctx, n, T, h_slots);
    return rc ? rc : tiny_sequence_internal(ctx, d_x, n, T, h_slots, d_out);
}

extern "C" int dt_tiny_stream_forward(dt_ctx *ctx, const float *d_feat, const float *d_det, int n, int T, int fh, int fw, int fc, int pool,
                                      const int *h_slots, float *d_out)
{
    if (!ctx || !d_feat || !d_det || !d_out) return dt_fail(ctx, DT_ERR_ARG, "null argument");
    int rc = tiny_stream_check(ctx, n, T, h_slots);      // before the features: an error launches nothing
    if (rc) return rc;
    float *rows = ws_get(ctx, "tiny_rows", (size_t)n * T * ctx->tiny_D * sizeof(float));
    if (!rows) return DT_ERR_DEVICE;
    rc = dt_tiny_features(ctx, d_feat, d_det, n * T, fh, fw, fc, pool, rows);
    return rc ? rc : tiny_sequence_internal(ctx, rows, n, T, h_slots, d_out);
}

extern "C" int dt_tiny_forward(dt_ctx *ctx, const float *d_feat, const float *d_det, int n_seq, int T, int fh, int fw,
                               int fc, int pool, float *d_out)
{
    if (!ctx) return DT_ERR_ARG;
    if (!ctx->tiny_loaded) return dt_fail(ctx, DT_ERR_STATE, "TinyTracker weights not loaded");
    float *rows = ws_get(ctx, "tiny_rows", (size_t)n_seq * T * ctx->tiny_D * sizeof(float));
    if (!rows) return DT_ERR_DEVICE;
    int rc = dt_tiny_features(ctx, d_feat, d_det, n_seq * T, fh, fw, fc, pool, rows);
    if (rc) return rc;
    return dt_tiny_sequence(ctx, rows, n_seq, T, d_out);
}

// generate_heatmap_feat (utility/utils.py:53-58) for n centre-format boxes and
// generate_rectangle_from_heatmap (utility/utils.py:61-79)
extern "C" int dt_heatmap_from_boxes(dt_ctx *ctx, const float *d_box4, int n, int hmap_size, float *d_heat)
{
    if (!ctx || !d_box4 || !d_heat || hmap_size < 1) return dt_fail(ctx, DT_ERR_ARG, "bad argument");
    if (launch_heatmap_from_boxes(ctx->stream, d_box4, nullptr, n, hmap_size, d_heat))
        return dt_fail(ctx, DT_ERR_DEVICE, "heatmap launch failed");
    return DT_OK;
}

extern "C" int dt_heatmap_from_xywh64(dt_ctx *ctx, const double *d_xywh, int n, int hmap_size, float *d_heat)
{
    if (!ctx || !d_xywh || !d_heat || hmap_size < 1) return dt_fail(ctx, DT_ERR_ARG, "bad argument");
    if (launch_heatmap_from_boxes(ctx->stream, nullptr, d_xywh, n, hmap_size, d_heat))
        return dt_fail(ctx, DT_ERR_DEVICE, "heatmap launch failed");
    return DT_OK;
}

extern "C" int dt_encode_targets(dt_ctx *ctx, const int *d_objs, const int *d_counts, const int *d_dims,
                                 const double *d_aug, int n_frames, int cap, int grid_h, int grid_w, int nb_box,
                                 int nb_class, int image_h, int image_w, int true_box_buffer,
                                 const double *h_anchors, double *d_y, double *d_b)
{
    if (!ctx || !d_objs || !d_counts || !d_dims || !h_anchors || !d_y || !d_b || n_frames < 0)
        return dt_fail(ctx, DT_ERR_ARG, "bad argument");
    ProfScope ps(ctx, "encode_targets", 0.0,
                 8.0 * n_frames * ((double)grid_h * grid_w * nb_box * (5 + nb_class) + 4.0 * true_box_buffer) +
                     20.0 * n_frames * cap,
                 nullptr);
    const int rc = launch_encode_targets(ctx->stream, d_objs, d_counts, d_dims, d_aug, n_frames, cap, grid_h, grid_w,
                                         nb_box, nb_class, image_h, image_w, true_box_buffer, h_anchors, d_y, d_b);
    if (rc == 2) return dt_fail(ctx, DT_ERR_ARG, "encode_targets: unsupported shape (nb_box <= %d)", DT_MAX_ANCHOR_BOXES);
    if (rc) return dt_fail(ctx, DT_ERR_DEVICE, "encode_targets launch failed");
    return DT_OK;
}

extern "C" int dt_rect_from_heatmap(dt_ctx *ctx, const float *d_heat, int n, int hmap_size, float thresh, int *d_rect)
{
    if (!ctx || !d_heat || !d_rect || hmap_size < 1) return dt_fail(ctx, DT_ERR_ARG, "bad argument");
    if (launch_rect_from_heatmap(ctx->stream, d_heat, n, hmap_size, thresh, d_rect))
        return dt_fail(ctx, DT_ERR_DEVICE, "rect_from_heatmap launch failed");
    return DT_OK;
}

// detection box fed to the single-object tracker: the highest-score survivor of a frame
// as (cx, cy, w, h) in image-relative units (preprocessing.py:441-444), zeros if none
extern "C" int dt_top_box(dt_ctx *ctx, const float *d_boxes, const int *d_counts, int n_frames, int cap, float *d_out4)
{
    if (!ctx || !d_boxes || !d_counts || !d_out4) return dt_fail(ctx, DT_ERR_ARG, "null argument");
    if (launch_top_box(ctx->stream, d_boxes, d_counts, n_frames, cap, d_out4))
        return dt_fail(ctx, DT_ERR_DEVICE, "top_box launch failed");
    return DT_OK;
}

// ---------------------------------------------------------------------------
// layer-level entry points for the parity tests
// ---------------------------------------------------------------------------
extern "C" int dt_conv2d(dt_ctx *ctx, const float *d_in, int B, int H, int W, int Cin, const float *h_kernel, int k,
                         int Cout, const float *h_bias, float leaky_slope, int pool, float *d_out, float *d_out2)
{
    if (ctx) call_begin(ctx, 0);
    if (!ctx || !d_in || !h_kernel || !d_out) return dt_fail(ctx, DT_ERR_ARG, "null argument");
    if (Cin % 32) return dt_fail(ctx, DT_ERR_ARG, "Cin must be a multiple of 32");
    if (k != 1 && k != 3) return dt_fail(ctx, DT_ERR_ARG, "kernel size must be 1 or 3");
    if (pool && ((H | W) & 1)) return dt_fail(ctx, DT_ERR_ARG, "pooling needs even H and W");
    policy_refresh(ctx);   // test entry point: the parity tests force policies on a live context through the environment
    std::vector<float> zero(Cout, 0.0f);
    int rc = load_conv_layer(ctx, 0, k, Cin, Cout, h_kernel, nullptr, h_bias ? h_bias : zero.data());
    if (rc) return rc;
    const ConvLayer &L = ctx->layers[0];
    switch (pool) {
    case 0: return run_conv(ctx, L, d_in, Cin, B, H, W, d_out, Cout, ORD_LINEAR, EPI_PLAIN, leaky_slope);
    case 1: return run_conv(ctx, L, d_in, Cin, B, H, W, d_out, Cout, ORD_QUAD, EPI_POOL, leaky_slope);
    case 2:
        if (!d_out2 || k != 3) return dt_fail(ctx, DT_ERR_ARG, "pool=2 needs d_out2 and k=3");
        return run_conv(ctx, L, d_in, Cin, B, H, W, d_out, Cout, ORD_QUAD, EPI_POOL_BOTH, leaky_slope, d_out2, Cout);
    case 3:
        if (k != 1) return dt_fail(ctx, DT_ERR_ARG, "space_to_depth epilogue needs k=1");
        return run_conv(ctx, L, d_in, Cin, B, H, W, d_out, 4 * Cout, ORD_QUAD, EPI_S2D, leaky_slope);
    default: return dt_fail(ctx, DT_ERR_ARG, "bad pool mode");
    }
}

namespace {
// A test entry point keeps its device temporaries in DevMem / WinoWeights locals and declares one of these BEHIND them: on every return path
// the stream is idle before they are released
struct SyncAtExit {
    hipStream_t st;
    ~SyncAtExit() { (void)hipStreamSynchronize(st); }
};
}   // namespace

extern "C" int dt_convlstm_step(dt_ctx *ctx, const float *d_x, int B, int H, int W, int Cx, const float *d_h,
                                const float *d_c, int U, const float *h_kernel, const float *h_recurrent,
                                const float *h_bias, float *d_h_out, float *d_c_out)
{
    if (ctx) call_begin(ctx, 0);
    if (!ctx || !d_x || !d_h || !d_c || !h_kernel || !h_recurrent || !h_bias || !d_h_out || !d_c_out)
        return dt_fail(ctx, DT_ERR_ARG, "null argument");
    if (Cx % 32 || U % 32) return dt_fail(ctx, DT_ERR_ARG, "Cx and U must be multiples of 32");
    policy_refresh(ctx);   // test entry point (see dt_conv2d)
    const int N4 = 4 * U, GG = H * W;
    std::vector<int> n_map;
    gate_interleave_map(U, n_map);
    std::vector<float> wx((size_t)N4 * 9 * Cx), wh((size_t)N4 * 9 * U), bx(N4);
    pack_conv_weights(h_kernel, 3, Cx, N4, nullptr, Cx, n_map.data(), N4, nullptr, wx.data());
    pack_conv_weights(h_recurrent, 3, U, N4, nullptr, U, n_map.data(), N4, nullptr, wh.data());
    for (int np = 0; np < N4; ++np) bx[np] = h_bias[n_map[np]];
    DevMem<float> dwx, dwh, dbx;
    WinoWeights uwx, uwh;
    SyncAtExit idle{ctx->stream};
    int rc;
    if ((rc = upload(ctx, dwx, wx)) || (rc = upload(ctx, dwh, wh)) || (rc = upload(ctx, dbx, bx))) return rc;
    float *xproj = ws_get(ctx, "cl_xproj", (size_t)B * GG * N4 * sizeof(float));
    if (!xproj) return DT_ERR_DEVICE;
    if (ctx->pol.wino == 2 && wino_wanted(ctx, 3, Cx, N4) && wino_wanted(ctx, 3, U, N4)) {   // the same step through the Winograd path
        const int ts = wino_tile(ctx, false);
        if ((rc = upload_wino(ctx, uwx, ts, h_kernel, Cx, N4, nullptr, Cx, n_map.data(), N4, nullptr, ts == 6)) ||
            (rc = upload_wino(ctx, uwh, ts, h_recurrent, U, N4, nullptr, U, n_map.data(), N4, nullptr, ts == 4)))
            return rc;
        WinoIO io;
        memset(&io, 0, sizeof(io));
        io.in = d_x; io.in_ld = Cx; io.in_bs = (long long)GG * Cx;
        io.out = xproj; io.out_ld = N4; io.out_bs = (long long)GG * N4;
        if ((rc = run_wino(ctx, uwx, choose_wino(ctx, uwx, N4, B, H, W, io), dbx.get(), N4, B, H, W, io, 1.0f, "convlstm_xproj", 0, AMAX_TEST))) return rc;
        HIP_TRY(ctx, hipMemcpyAsync(d_c_out, d_c, (size_t)B * GG * U * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
        memset(&io, 0, sizeof(io));
        io.in = d_h; io.in_ld = U; io.in_bs = (long long)GG * U;
        io.out = d_h_out; io.out_ld = U; io.out_bs = (long long)GG * U;
        io.xproj = xproj; io.xp_ld = N4; io.xp_bs = (long long)GG * N4;
        io.cstate = d_c_out; io.c_ld = U; io.c_bs = (long long)GG * U;
        return run_wino(ctx, uwh, choose_wino(ctx, uwh, N4, B, H, W, io), nullptr, N4, B, H, W, io, 1.0f, "convlstm_step", 0, AMAX_TEST + 1);      // (a caller's h: measured)
    }
    ConvArgs a;
    memset(&a, 0, sizeof(a));
    a.in = d_x; a.in_ld = Cx; a.in_bs = (long long)GG * Cx;
    a.wt = dwx.get(); a.bias = dbx.get();
    a.out = xproj; a.out_ld = N4; a.out_bs = (long long)GG * N4;
    a.B = B; a.H = H; a.W = W; a.Cin = Cx; a.N = N4; a.M = B * GG; a.K = 9 * Cx; a.slope = 1.0f;
    if (launch_igemm(ctx, a, 3, ORD_LINEAR, EPI_PLAIN, CFG_128x128))
        return dt_fail(ctx, DT_ERR_DEVICE, "xproj launch failed");
    HIP_TRY(ctx, hipMemcpyAsync(d_c_out, d_c, (size_t)B * GG * U * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
    memset(&a, 0, sizeof(a));
    a.in = d_h; a.in_ld = U; a.in_bs = (long long)GG * U;
    a.wt = dwh.get();
    a.out = d_h_out; a.out_ld = U; a.out_bs = (long long)GG * U;
    a.xproj = xproj; a.xp_ld = N4; a.xp_bs = (long long)GG * N4;
    a.cstate = d_c_out; a.c_ld = U; a.c_bs = (long long)GG * U;
    a.B = B; a.H = H; a.W = W; a.Cin = U; a.N = N4; a.M = B * GG; a.K = 9 * U; a.slope = 1.0f;
    if (launch_igemm(ctx, a, 3, ORD_LINEAR, EPI_GATES, CFG_128x128))
        return dt_fail(ctx, DT_ERR_DEVICE, "gates launch failed");
    return DT_OK;
}

// wino_gemm_s3.hip on caller data (parity tests at the benched shapes): both operands padded to the kernel's row tiles, split by the
// production pack kernels -- nt = 3: three bf16 terms; nt = 2: two fp16 terms of the scaled operands (V by ONE power of two from its
// max |x| like an activation, U per plane like the weights) -- then the production launcher.
extern "C" int dt_gemm_split(dt_ctx *ctx, const float *d_v, const float *d_u, int P, int Mt, int K, int N, int half, int nt, float *d_m)
{
    if (!ctx || !d_v || !d_u || !d_m) return dt_fail(ctx, DT_ERR_ARG, "null argument");
    call_begin(ctx, 0);
    if (P <= 0 || Mt <= 0 || K <= 0 || N <= 0 || K % 32 || N % 128 || !wino_gemm_s3_usable(Mt, K, N) || (nt != 2 && nt != 3) || (nt == 2 && P > 64))
        return dt_fail(ctx, DT_ERR_ARG, "dt_gemm_split: unsupported shape P=%d Mt=%d K=%d N=%d nt=%d", P, Mt, K, N, nt);
    const bool rows_form = half == 2;      // the 1x1 layers' form: the kernel reads d_v as fp32 rows and splits its fragments itself
    if (rows_form && P != 1) return dt_fail(ctx, DT_ERR_ARG, "dt_gemm_split: the fp32-rows form is one GEMM (P = 1)");
    if (rows_form) half = 0;
    const size_t Mp = ((size_t)Mt + 255) / 256 * 256, Np = ((size_t)N + 255) / 256 * 256;
    DevMem<float> vpad, upad, ps;
    DevMem<unsigned short> vs, us;
    SyncAtExit idle{ctx->stream};
    HIP_TRY(ctx, vpad.alloc((size_t)P * Mp * K));
    HIP_TRY(ctx, upad.alloc((size_t)P * Np * K));
    HIP_TRY(ctx, vs.alloc((size_t)P * nt * Mp * K));
    HIP_TRY(ctx, us.alloc((size_t)P * nt * Np * K));
    HIP_TRY(ctx, ps.alloc(64));
    HIP_TRY(ctx, hipMemsetAsync(vpad.get(), 0, (size_t)P * Mp * K * sizeof(float), ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(upad.get(), 0, (size_t)P * Np * K * sizeof(float), ctx->stream));
    HIP_TRY(ctx, hipMemcpy2DAsync(vpad.get(), Mp * K * sizeof(float), d_v, (size_t)Mt * K * sizeof(float), (size_t)Mt * K * sizeof(float), P,
                                  hipMemcpyDeviceToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpy2DAsync(upad.get(), Np * K * sizeof(float), d_u, (size_t)N * K * sizeof(float), (size_t)N * K * sizeof(float), P,
                                  hipMemcpyDeviceToDevice, ctx->stream));
    GemmS3Args g;
    memset(&g, 0, sizeof(g));
    if (nt == 2) {
        unsigned *vslot = amax_slot(ctx, AMAX_TEST);
        if (launch_wino_h2_pack(ctx->stream, vpad.get(), P, (int)Mp, K, 0, vslot, vs.get(), nullptr) ||
            launch_wino_h2_pack(ctx->stream, upad.get(), P, (int)Np, K, 0, amax_slot(ctx, AMAX_PACK), us.get(), ps.get()))
            return dt_fail(ctx, DT_ERR_DEVICE, "fp16-form pack launch failed");
        g.nt = 2; g.pscale = ps.get(); g.amax = vslot;      // (the fp32-rows form measures the same tensor: the padding rows are zeros)
    } else if (launch_wino_s3_pack(ctx->stream, vpad.get(), P, (int)Mp, K, vs.get()) || launch_wino_s3_pack(ctx->stream, upad.get(), P, (int)Np, K, us.get()))
        return dt_fail(ctx, DT_ERR_DEVICE, "split-bf16 pack launch failed");
    g.a = vs.get(); g.b = us.get(); g.c = d_m;
    if (rows_form) { g.a = nullptr; g.a_f32 = d_v; g.a_ld = K; g.act = 1; g.slope = 1.0f; }      // (no bias, no activation)
    g.c_ps = (long long)Mt * N; g.P = P; g.Mt = Mt; g.Mp = (int)Mp; g.N = N; g.Np = (int)Np; g.K = K; g.ldc = N; g.half = half;
    ProfScope pscope(ctx, "conv_gemm_s3", wino_gemm_s3_flops(g), (double)P * (2.0 * nt * Mt * K + 2.0 * nt * (double)K * N + 4.0 * (double)Mt * N), "test_gemm");
    if (pscope.on) prof_count(ctx, wino_gemm_s3_half_chosen(g, 0) ? "s3_tile:128x2" : "s3_tile:256");
    const int rc = launch_wino_gemm_s3(ctx->stream, g, 0);
    if (rc) return dt_fail(ctx, launch_code(rc), "dt_gemm_split: launch failed (rc=%d)", rc);
    return DT_OK;
}
extern "C" int dt_gemm_split_bf16(dt_ctx *ctx, const float *d_v, const float *d_u, int P, int Mt, int K, int N, int half, float *d_m)
{
    return dt_gemm_split(ctx, d_v, d_u, P, Mt, K, N, half, 3, d_m);
}

// winograd.hip's transforms ALONE on caller data (tests/test_gpu_wino_transform.py): the production geometry rule, the production launchers, nothing else.
// h_geom[DT_WINO_GEOM_INTS] = g, ph, pw, th, tw, Mt, Mp, then what the launcher's choice function decided: form (WIN_* / WOUT_*), workgroups, threads.
static void wino_test_geometry(dt_ctx *ctx, int ts, int B, int H, int W, bool pooled, WinoArgs &w, int *h_geom)
{
    const WinoGeom q = wino_geometry(ctx, ts, B, H, W, pooled);
    w.B = B; w.H = H; w.W = W; w.ts = ts;
    w.g = q.g; w.ph = q.ph; w.pw = q.pw; w.th = q.th; w.tw = q.tw; w.Mt = q.Mt;
    w.Mp = (q.Mt + 255) / 256 * 256;
    const int geom[7] = {q.g, q.ph, q.pw, q.th, q.tw, q.Mt, w.Mp};
    memcpy(h_geom, geom, sizeof(geom));
    h_geom[7] = h_geom[8] = h_geom[9] = 0;
}
static void wino_test_report(const WinoLaunch &l, int *h_geom) { h_geom[7] = l.form; h_geom[8] = (int)l.grid; h_geom[9] = (int)l.threads; }
static bool wino_test_shape_ok(int ts, int B, int H, int W) { return (ts == 2 || ts == 4 || ts == 6) && B > 0 && H > 0 && W > 0 && (long long)B * H * W < (1ll << 24); }

extern "C" int dt_wino_geometry(dt_ctx *ctx, int ts, int B, int H, int W, int pooled, int *h_geom)
{
    if (!ctx || !h_geom) return dt_fail(ctx, DT_ERR_ARG, "null argument");
    if (!wino_test_shape_ok(ts, B, H, W)) return dt_fail(ctx, DT_ERR_ARG, "dt_wino_geometry: unsupported shape ts=%d B=%d H=%d W=%d", ts, B, H, W);
    policy_refresh(ctx);   // test entry point (see dt_conv2d)
    WinoArgs w{};
    wino_test_geometry(ctx, ts, B, H, W, pooled != 0, w, h_geom);
    return DT_OK;
}

extern "C" int dt_wino_input(dt_ctx *ctx, const float *d_in, int B, int H, int W, int C, int in_ld, long long in_bs, int ts, int pooled, int nt,
                             int force_form, int wg_cap, void *d_v, long long v_bytes, int *h_geom)
{
    if (!ctx || !d_in || !d_v || !h_geom) return dt_fail(ctx, DT_ERR_ARG, "null argument");
    call_begin(ctx, 0);
    if (!wino_test_shape_ok(ts, B, H, W) || C <= 0 || in_ld < C || in_bs < (long long)H * W * in_ld || in_bs % 4 || (nt != 0 && nt != 2 && nt != 3) || force_form < 0 ||
        force_form > 2 || wg_cap < 0)
        return dt_fail(ctx, DT_ERR_ARG, "dt_wino_input: unsupported arguments ts=%d B=%d H=%d W=%d C=%d in_ld=%d in_bs=%lld nt=%d force_form=%d wg_cap=%d", ts, B, H, W,
                       C, in_ld, in_bs, nt, force_form, wg_cap);
    policy_refresh(ctx);   // test entry point (see dt_conv2d)
    WinoArgs w{};
    wino_test_geometry(ctx, ts, B, H, W, pooled != 0, w, h_geom);
    const long long P = (ts + 2) * (ts + 2);
    const long long need = nt ? P * nt * w.Mp * C * (long long)sizeof(unsigned short) : P * w.Mt * C * (long long)sizeof(float);
    if (v_bytes < need) return dt_fail(ctx, DT_ERR_ARG, "dt_wino_input: V takes %lld bytes, the buffer has %lld", need, v_bytes);
    w.in = d_in; w.in_bs = in_bs; w.in_ld = in_ld; w.C = C;
    w.force_form = force_form; w.wg_cap = wg_cap;
    if (nt) { w.v_s3 = static_cast<unsigned short *>(d_v); w.nt = nt; }
    else w.v = static_cast<float *>(d_v);
    if (nt == 2) {      // V's power of two comes from the input's max |x|, measured into the test slot as run_wino does it (dense frames: ONE tensor of rows)
        if (in_bs != (long long)H * W * in_ld || C % 4) return dt_fail(ctx, DT_ERR_ARG, "dt_wino_input: the fp16 form measures B*H*W dense rows of C %% 4 == 0 channels");
        w.amax = ensure_amax(ctx, d_in, (long long)B * H * W, C, in_ld, AMAX_TEST);
        if (!w.amax) return DT_ERR_DEVICE;
    }
    const WinoLaunch l = choose_wino_input(w);
    if (!l.form) return dt_fail(ctx, DT_ERR_ARG, "dt_wino_input: the launcher refuses ts=%d C=%d in_ld=%d nt=%d (C %% 4, the split forms' C %% 32 / C %% 16 and tile sizes)", ts, C, in_ld, nt);
    wino_test_report(l, h_geom);
    const int rc = launch_wino_input(ctx->stream, w);
    if (rc) return dt_fail(ctx, launch_code(rc), "dt_wino_input: launch failed (rc=%d)", rc);
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return DT_OK;
}

extern "C" int dt_wino_output(dt_ctx *ctx, const float *d_m, long long m_floats, int m_ld, int N, int B, int H, int W, int ts, const float *d_bias,
                              const float *d_bias16, float slope, float *d_out, int out_ld, float *d_out2, int out2_ld, int publish, const float *d_xproj, int xp_ld,
                              float *d_cstate, int c_ld, int force_form, int wg_cap, int *h_geom)
{
    if (!ctx || !d_m || !h_geom || (!d_out && !d_out2)) return dt_fail(ctx, DT_ERR_ARG, "null argument");
    call_begin(ctx, 0);
    const bool gates = d_cstate != nullptr;
    if (!wino_test_shape_ok(ts, B, H, W) || N <= 0 || m_ld < N || force_form < 0 || force_form > 2 || wg_cap < 0 || (d_out && out_ld < (gates ? N / 4 : N)) ||
        (d_out2 && out2_ld < N))
        return dt_fail(ctx, DT_ERR_ARG, "dt_wino_output: unsupported arguments ts=%d B=%d H=%d W=%d N=%d m_ld=%d out_ld=%d out2_ld=%d force_form=%d wg_cap=%d", ts, B, H, W,
                       N, m_ld, out_ld, out2_ld, force_form, wg_cap);
    if (gates && (!d_xproj || !d_out || d_out2 || d_bias || d_bias16 || publish || xp_ld < N || c_ld < N / 4))
        return dt_fail(ctx, DT_ERR_ARG, "dt_wino_output: the gate form takes xproj [..][xp_ld >= N], cstate [..][c_ld >= N/4] and h (d_out) alone");
    policy_refresh(ctx);   // test entry point (see dt_conv2d)
    WinoArgs w{};
    wino_test_geometry(ctx, ts, B, H, W, d_out2 != nullptr, w, h_geom);
    const long long P = (ts + 2) * (ts + 2), need = P * w.Mt * m_ld;
    if (m_floats < need) return dt_fail(ctx, DT_ERR_ARG, "dt_wino_output: M' takes %lld floats, the buffer has %lld", need, m_floats);
    w.m = d_m; w.m_ld = m_ld; w.N = N; w.bias = d_bias; w.bias16 = d_bias16; w.slope = slope;
    w.out = d_out; w.out_ld = out_ld; w.out_bs = (long long)H * W * out_ld; w.out2 = d_out2; w.out2_ld = out2_ld;
    w.xproj = d_xproj; w.xp_ld = xp_ld; w.xp_bs = (long long)H * W * xp_ld;
    w.cstate = d_cstate; w.c_ld = c_ld; w.c_bs = (long long)H * W * c_ld;
    w.force_form = force_form; w.wg_cap = wg_cap;
    if (publish) {
        w.amax_out = amax_slot(ctx, AMAX_TEST);
        if (!w.amax_out) return dt_fail(ctx, DT_ERR_STATE, "max-|x| slots not allocated");
        HIP_TRY(ctx, hipMemsetAsync(w.amax_out, 0, DT_AMAX_WORDS * sizeof(unsigned), ctx->stream));
    }
    const WinoLaunch l = choose_wino_output(w, gates);
    if (!l.form)
        return dt_fail(ctx, DT_ERR_ARG, "dt_wino_output: the launcher refuses ts=%d N=%d m_ld=%d out_ld=%d out2_ld=%d slope=%g%s (N %% 4, N %% 128 for gates, row strides %% 4; "
                       "bias16 needs slope 1, a full-resolution output and no pooling)", ts, N, m_ld, out_ld, out2_ld, (double)slope, d_bias16 ? " bias16" : "");
    wino_test_report(l, h_geom);
    const int rc = launch_wino_output(ctx->stream, w, gates);
    if (rc) return dt_fail(ctx, launch_code(rc), "dt_wino_output: launch failed (rc=%d)", rc);
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return DT_OK;
}

// conv_igemm.hip ALONE on caller views (tests/test_gpu_conv_igemm_edges.py): the production weight packing, the production launcher with the tile
// configuration it is handed (force_cfg = 0: no policy reaches it), and -- for split-K -- the slab and the reduce kernel as conv_igemm() above runs
// them.  h_info = what plan_conv_igemm, the function the launcher itself dispatches on, resolved.
static_assert(DT_CONV_PLAIN == EPI_PLAIN && DT_CONV_POOL == EPI_POOL && DT_CONV_POOL_BOTH == EPI_POOL_BOTH && DT_CONV_S2D == EPI_S2D && DT_CONV_GATES == EPI_GATES &&
                  DT_CONV_PARTIAL == EPI_PARTIAL && DT_CFG_128x128 == CFG_128x128 && DT_CFG_128x64 == CFG_128x64 && DT_CFG_256x128 == CFG_256x128 &&
                  DT_CFG_256x256 == CFG_256x256 && DT_CFG_64x128 == CFG_64x128,
              "the codes dt_conv_igemm takes and reports (mi355_dt.h)");
extern "C" int dt_conv_igemm(dt_ctx *ctx, const dt_conv_igemm_desc *desc, const float *d_in, const float *h_kernel, const float *h_bias, const float *d_wt,
                             float *d_out, float *d_out2, const float *d_xproj, float *d_cstate, int *h_info)
{
    if (!ctx || !desc || !d_in || !d_out || !h_info) return dt_fail(ctx, DT_ERR_ARG, "null argument");
    call_begin(ctx, 0);
    const dt_conv_igemm_desc &d = *desc;
    const int ks = d.ks, B = d.B, H = d.H, W = d.W, Cin = d.Cin, N = d.N, P = d.P > 1 ? d.P : 1;
    const bool batched = P > 1, gates = d.kind == DT_CONV_GATES, split = d.kind == DT_CONV_PARTIAL || d.ksplit > 1;
    const int epi = split ? EPI_PARTIAL : d.kind, order = (epi == EPI_POOL || epi == EPI_POOL_BOTH || epi == EPI_S2D) ? ORD_QUAD : ORD_LINEAR;
    const int ksplit = d.ksplit > 1 ? d.ksplit : 1;
    memset(h_info, 0, DT_CONV_INFO_INTS * sizeof(int));
    if ((ks != 1 && ks != 3) || B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || N <= 0 || (long long)B * H * W >= (1ll << 24) || d.in_ld < Cin ||
        d.in_bs < (long long)H * W * d.in_ld || d.kind < DT_CONV_PLAIN || d.kind > DT_CONV_PARTIAL || d.cfg < 0 || d.cfg > CFG_64x128 || d.wg_cap < 0 || d.ksplit < 0 ||
        (d.act != 0 && d.act != 1) || (split && d.kind != DT_CONV_PLAIN && d.kind != DT_CONV_PARTIAL) || (long long)ksplit * 32 > (long long)ks * ks * Cin ||
        (d.npad != 0 && (d.npad % 128 || d.npad < N)) || ((d.publish || d.act) && (split || gates)))
        return dt_fail(ctx, DT_ERR_ARG, "dt_conv_igemm: unsupported arguments ks=%d B=%d H=%d W=%d Cin=%d N=%d in_ld=%d in_bs=%lld kind=%d cfg=%d ksplit=%d npad=%d wg_cap=%d",
                       ks, B, H, W, Cin, N, d.in_ld, (long long)d.in_bs, d.kind, d.cfg, d.ksplit, d.npad, d.wg_cap);
    const int out_cols = gates ? N / 4 : (epi == EPI_S2D ? 4 * N : N);
    if (d.out_ld < out_cols || (epi == EPI_POOL_BOTH && (!d_out2 || d.out2_ld < N)) || (epi != EPI_POOL_BOTH && d_out2))
        return dt_fail(ctx, DT_ERR_ARG, "dt_conv_igemm: kind %d writes %d columns to d_out (out_ld=%d) and %s d_out2 (out2_ld=%d)", d.kind, out_cols, d.out_ld,
                       epi == EPI_POOL_BOTH ? "the pooled tensor to" : "has no", d.out2_ld);
    if (gates ? (N % 128 || !d_xproj || !d_cstate || h_bias || d.xp_ld < N || d.c_ld < N / 4 || d.slope != 1.0f) : (d_xproj || d_cstate))
        return dt_fail(ctx, DT_ERR_ARG, "dt_conv_igemm: the gate kind takes N = 4 U (U %% 32 == 0), xproj [..][xp_ld >= N], cstate [..][c_ld >= U], no bias; no other kind takes them");
    if (batched ? (ks != 1 || d.kind != DT_CONV_PLAIN || split || B != 1 || H != 1 || !d_wt || h_kernel || h_bias || d.in_ld != Cin || d.in_bs != (long long)W * Cin)
                : (!h_kernel || d_wt))
        return dt_fail(ctx, DT_ERR_ARG, "dt_conv_igemm: P > 1 is the batched GEMM (ks 1, plain, B = H = 1, W = Mt, dense [P][Mt][Cin] and d_wt [P][N][Cin], no bias); "
                                        "P <= 1 takes h_kernel");
    const int K = ks * ks * Cin, M = B * H * W;
    const int npad = gates ? N : (d.npad ? d.npad : round_up(N, 256));
    ConvArgs a{};
    a.in = d_in; a.in_ld = d.in_ld; a.in_bs = d.in_bs;
    a.out = d_out; a.out_ld = d.out_ld; a.out_bs = (long long)H * W * d.out_ld;
    a.out2 = d_out2; a.out2_ld = d.out2_ld;
    a.xproj = d_xproj; a.xp_ld = d.xp_ld; a.xp_bs = (long long)H * W * d.xp_ld;
    a.cstate = d_cstate; a.c_ld = d.c_ld; a.c_bs = (long long)H * W * d.c_ld;
    a.B = B; a.H = H; a.W = W; a.Cin = Cin; a.N = N; a.M = M; a.K = K;
    a.npad = gates ? 0 : npad; a.slope = d.slope; a.act = d.act; a.wg_cap = d.wg_cap;
    if (batched) {      // as run_wino fills it
        a.out_bs = (long long)M * d.out_ld;
        a.zbatch = P; a.z_in = (long long)M * Cin; a.z_wt = (long long)npad * K; a.z_out = (long long)M * d.out_ld;
    }
    if (split) { a.out_ld = N; a.ksplit = ksplit; }      // as conv_igemm() above: raw partial sums to a dense slab, bias and activation in the reduce
    // the launcher's own verdict BEFORE anything is packed or allocated (pack_conv_weights relies on Cin % 32 == 0)
    const ConvPlan pl = plan_conv_igemm(a, ks, order, epi, d.cfg);
    if (pl.rc) return dt_fail(ctx, DT_ERR_ARG, "dt_conv_igemm: the launcher refuses ks=%d kind=%d H=%d W=%d Cin=%d in_ld=%d in_bs=%lld (Cin %% 32, even H and W for the "
                                               "quad kinds, dense frames for a 1x1 linear launch)", ks, d.kind, H, W, Cin, d.in_ld, (long long)d.in_bs);
    const int info[DT_CONV_INFO_INTS] = {pl.cfg, pl.bm, pl.bn, pl.threads, pl.persist, pl.grid_x, pl.grid_y, pl.total};
    memcpy(h_info, info, sizeof(info));
    std::vector<float> packed, bias;
    std::vector<int> n_map;
    DevMem<float> wt, bs, slab;
    SyncAtExit idle{ctx->stream};
    int rc;
    if (batched) {      // [P][N][K] -> [P][npad][K], the rows behind N zero (as upload_wino pads U)
        HIP_TRY(ctx, wt.alloc((size_t)P * npad * K));
        HIP_TRY(ctx, hipMemsetAsync(wt.get(), 0, (size_t)P * npad * K * sizeof(float), ctx->stream));
        HIP_TRY(ctx, hipMemcpy2DAsync(wt.get(), (size_t)npad * K * sizeof(float), d_wt, (size_t)N * K * sizeof(float), (size_t)N * K * sizeof(float), P,
                                      hipMemcpyDeviceToDevice, ctx->stream));
    } else {
        packed.resize((size_t)npad * K);
        if (gates) gate_interleave_map(N / 4, n_map);      // as dt_convlstm_step / dt_tracker_load pack the recurrent kernel
        pack_conv_weights(h_kernel, ks, Cin, N, nullptr, Cin, gates ? n_map.data() : nullptr, npad, nullptr, packed.data());
        if ((rc = upload(ctx, wt, packed))) return rc;
        if (h_bias) {      // padded to npad, as load_conv_layer does
            bias.assign((size_t)npad, 0.0f);
            for (int c = 0; c < N; ++c) bias[c] = h_bias[c];
            if ((rc = upload(ctx, bs, bias))) return rc;
        }
    }
    a.wt = wt.get(); a.bias = (h_bias && !split) ? bs.get() : nullptr;
    if (split) {
        HIP_TRY(ctx, slab.alloc((size_t)ksplit * M * N));
        a.out = slab.get();
    }
    if (d.publish) {
        a.amax_out = amax_slot(ctx, AMAX_TEST);
        if (!a.amax_out) return dt_fail(ctx, DT_ERR_STATE, "max-|x| slots not allocated");
        HIP_TRY(ctx, hipMemsetAsync(a.amax_out, 0, DT_AMAX_WORDS * sizeof(unsigned), ctx->stream));
    }
    rc = launch_conv_igemm(ctx->stream, a, ks, order, epi, d.cfg);
    if (rc) return dt_fail(ctx, launch_code(rc), "dt_conv_igemm: launch failed (rc=%d)", rc);
    if (split && launch_splitk_reduce(ctx->stream, slab.get(), ksplit, M, N, h_bias ? bs.get() : nullptr, d.slope, d_out, d.out_ld))
        return dt_fail(ctx, DT_ERR_DEVICE, "dt_conv_igemm: split-K reduce launch failed");
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return DT_OK;
}

// conv1.hip ALONE (tests/test_gpu_conv1_edges.py): the production split tables (upload_conv1_tables), the context's x/255 table and the production
// launcher, with no detector configured and no policy.  h_info = what plan_conv1, the function the launcher itself dispatches on, resolved.
static_assert(DT_C1_MFMA_F32 == C1_MFMA_F32 && DT_C1_S3_U8_FULL == C1_S3_U8_FULL && DT_C1_S3_U8 == C1_S3_U8 && DT_C1_S3_F32 == C1_S3_F32,
              "the instance codes dt_conv1 reports (mi355_dt.h)");
extern "C" int dt_conv1(dt_ctx *ctx, const void *d_frames, int frames_dtype, int B, int H, int W, const float *h_w, const float *h_bias, float slope,
                        int split, int tpw, int publish, float *d_out, int *h_info)
{
    if (!ctx || !d_frames || !h_w || !h_bias || !d_out || !h_info) return dt_fail(ctx, DT_ERR_ARG, "null argument");
    call_begin(ctx, 0);
    memset(h_info, 0, DT_CONV1_INFO_INTS * sizeof(int));
    if (frames_dtype == DT_FRAMES_F32 && (reinterpret_cast<uintptr_t>(d_frames) & 3))
        return dt_fail(ctx, DT_ERR_ARG, "dt_conv1: float32 frames at an address that is no multiple of 4");
    const Conv1Plan pl = plan_conv1(d_frames, frames_dtype, B, H, W, slope, split != 0, tpw);
    if (pl.rc)
        return dt_fail(ctx, DT_ERR_ARG, "dt_conv1: the launcher refuses dtype=%d B=%d H=%d W=%d slope=%g tpw=%d (uint8 or float32 frames, even H and W, "
                                        "B in 1..65535, slope >= 0, tpw in 0..26)", frames_dtype, B, H, W, (double)slope, tpw);
    const int info[DT_CONV1_INFO_INTS] = {pl.inst, pl.tpw, pl.grid_x, pl.grid_y, pl.grid_z, pl.fills_amax};
    memcpy(h_info, info, sizeof(info));
    DevMem<float> w, bs;
    DevMem<unsigned> w3, w3u8;
    SyncAtExit idle{ctx->stream};
    int rc;
    if ((rc = upload(ctx, w, std::vector<float>(h_w, h_w + 27 * 32))) || (rc = upload(ctx, bs, std::vector<float>(h_bias, h_bias + 32)))) return rc;
    if (split && (rc = upload_conv1_tables(ctx, h_w, w3, w3u8))) return rc;
    unsigned *am = nullptr;
    if (publish) {
        am = amax_slot(ctx, AMAX_TEST);
        if (!am) return dt_fail(ctx, DT_ERR_STATE, "max-|x| slots not allocated");
        HIP_TRY(ctx, hipMemsetAsync(am, 0, DT_AMAX_WORDS * sizeof(unsigned), ctx->stream));
    }
    rc = launch_conv1_direct(ctx->stream, d_frames, frames_dtype, B, H, W, w.get(), bs.get(), ctx->lut255.get(), slope, d_out, split ? w3.get() : nullptr,
                             split ? w3u8.get() : nullptr, am, tpw);
    if (rc) return dt_fail(ctx, launch_code(rc), "dt_conv1: launch failed (rc=%d)", rc);
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return DT_OK;
}

// Re-reads the tuning / test knobs from the environment into the context (they are otherwise read in dt_create and by the
// layer-level test entry points); the context's pin override stays.  Knobs that shape the uploaded weights (DT_WINO, DT_WINO_TILE)
// take effect at the next weight load.
extern "C" int dt_policy_reload(dt_ctx *ctx)
{
    if (!ctx) return DT_ERR_ARG;
    policy_refresh(ctx);
    return DT_OK;
}

// One knob of ONE context, without going through the process environment (which other contexts and threads share):
//   "pin" 1 / 0 / -1 : kernel selection independent of the batch (DT_PIN; parallel.py: deterministic=True) on / off / as DT_PIN says.
//                      The override holds for the context's life, through every later re-read of the environment.
extern "C" int dt_policy_set(dt_ctx *ctx, const char *name, int value)
{
    if (!ctx || !name) return DT_ERR_ARG;
    if (strcmp(name, "pin") != 0) return dt_fail(ctx, DT_ERR_ARG, "dt_policy_set: unknown knob '%s'", name);
    if (value < -1 || value > 1) return dt_fail(ctx, DT_ERR_ARG, "dt_policy_set: pin must be -1, 0 or 1 (got %d)", value);
    ctx->pin_override = value;
    policy_refresh(ctx);
    return DT_OK;
}

// ---------------------------------------------------------------------------
// profiling
// ---------------------------------------------------------------------------
static void prof_drain(dt_ctx *ctx)
{
    (void)hipStreamSynchronize(ctx->stream);
    for (auto &e : ctx->pending) {
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, e.a, e.b) == hipSuccess) {
            ctx->prof_tab[e.name].ms += ms;
            if (!e.tag.empty()) ctx->prof_tab[e.tag].ms += ms;
        }
        (void)hipEventDestroy(e.a);
        (void)hipEventDestroy(e.b);
    }
    ctx->pending.clear();
}

extern "C" int dt_profile_enable(dt_ctx *ctx, int on)
{
    if (!ctx) return DT_ERR_ARG;
    prof_drain(ctx);
    ctx->prof = on != 0;
    return DT_OK;
}

extern "C" int dt_profile_reset(dt_ctx *ctx)
{
    if (!ctx) return DT_ERR_ARG;
    prof_drain(ctx);
    ctx->prof_tab.clear();
    return DT_OK;
}

extern "C" int dt_profile_names(dt_ctx *ctx, char *buf, size_t buflen)
{
    if (!ctx || !buf || !buflen) return DT_ERR_ARG;
    prof_drain(ctx);
    std::string all;
    for (auto &kv : ctx->prof_tab) { all += kv.first; all += "\n"; }
    if (all.size() + 1 > buflen) return dt_fail(ctx, DT_ERR_ARG, "dt_profile_names: buffer too small (%zu needed)", all.size() + 1);
    memcpy(buf, all.c_str(), all.size() + 1);
    return DT_OK;
}

extern "C" int dt_profile_read(dt_ctx *ctx, const char *name, int64_t *launches, double *total_ms, double *flops,
                               double *bytes)
{
    if (!ctx || !name) return DT_ERR_ARG;
    prof_drain(ctx);
    auto it = ctx->prof_tab.find(name);
    ProfEntry e;
    if (it != ctx->prof_tab.end()) e = it->second;
    if (!strcmp(name, "graph_replay")) e.launches = ctx->graph_replays;        // counters of the hipGraph path
    if (!strcmp(name, "graph_capture")) e.launches = ctx->graph_captures;
    if (launches) *launches = e.launches;
    if (total_ms) *total_ms = e.ms;
    if (flops) *flops = e.flops;
    if (bytes) *bytes = e.bytes;
    return DT_OK;
}
