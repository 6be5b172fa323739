// ModelHost: the host-side plumbing that vsc_encoder (encoder.hip) and vsc_swin (swin_encoder.hip) share -- the table of expected
// tensors and their host copies, tracked device allocations and the two uploads, the two lanes with their fork / join, and the
// per-launch event profiler.  No kernel, no virtual function; each model derives from it and keeps its own weights, workspaces,
// config checks, finalize body and launch sequence.
#pragma once
#include <map>
#include <string>
#include <vector>

#include "common.h"

struct ModelHost {
    const char *tag;   // "encoder" / "swin":  "<tag>: hipMalloc(..) failed"
    const char *api;   // ""        / "swin ": "<api>set_weight: ..", so that every error text stays what it was per model
    ModelHost(const char *tag_, const char *api_) : tag(tag_), api(api_) {}
    ModelHost(const ModelHost &) = delete;

    // ---- expected tensors and their host copies (ordered: finalize names the lexicographically first missing one) ----
    bool finalized = false;
    std::map<std::string, size_t> expected;
    std::map<std::string, std::vector<float>> host_w;

    void expect(const std::string &name, size_t count) { expected[name] = count; }
    int set_weight(const char *name, const float *host, size_t count) {
        if (finalized) {
            vsc_set_error("%sset_weight(%s) after finalize", api, name);
            return VSC_ERR_STATE;
        }
        auto it = expected.find(name);
        VSC_REQUIRE(it != expected.end(), "%sset_weight: unknown tensor '%s' for this config", api, name);
        VSC_REQUIRE(it->second == count, "%sset_weight: '%s' has %zu elements, expected %zu", api, name, count, it->second);
        host_w[name].assign(host, host + count);
        return VSC_OK;
    }
    int all_set() const {
        for (auto &kv : expected)
            if (!host_w.count(kv.first)) {
                vsc_set_error("%sfinalize: weight '%s' was never set", api, kv.first.c_str());
                return VSC_ERR_STATE;
            }
        return VSC_OK;
    }
    void drop_host() {
        host_w.clear();
        finalized = true;
    }
    int forward_ready() const {
        if (finalized) return VSC_OK;
        vsc_set_error("%sforward before finalize", api);
        return VSC_ERR_STATE;
    }

    // ---- device memory, freed with the handle ----
    std::vector<void *> allocs;

    int alloc(size_t bytes, void **out) {
        hipError_t err = hipMalloc(out, bytes);
        if (err != hipSuccess) {
            vsc_set_error("%s: hipMalloc(%zu) failed: %s", tag, bytes, hipGetErrorString(err));
            return VSC_ERR_NOMEM;
        }
        allocs.push_back(*out);
        return VSC_OK;
    }
    int upload_f32(const std::vector<float> &v, float **out) {
        VSC_TRY(alloc(v.size() * 4, (void **)out));
        VSC_CHECK_HIP(hipMemcpy(*out, v.data(), v.size() * 4, hipMemcpyHostToDevice));
        return VSC_OK;
    }
    int upload_f32(const std::string &name, float **out) { return upload_f32(host_w.at(name), out); }
    // f32 host matrix [rows, cols] -> device [rows, cols_pad] in the 16-bit operand type (zero padded); `name` is for the message
    int upload_bf16(const std::vector<float> &v, const std::string &name, int64_t rows, int cols, int cols_pad, uint16_t **out) {
        float *tmp = nullptr;
        VSC_CHECK_HIP(hipMalloc((void **)&tmp, v.size() * 4));
        hipError_t err = hipMemcpy(tmp, v.data(), v.size() * 4, hipMemcpyHostToDevice);
        int rc = err == hipSuccess ? alloc((size_t)rows * cols_pad * 2, (void **)out) : VSC_ERR_HIP;
        if (!rc) rc = launch_f32_to_bf16(tmp, *out, rows, cols, cols_pad, nullptr);
        hipError_t e2 = hipDeviceSynchronize();
        (void)hipFree(tmp);
        if (err != hipSuccess || e2 != hipSuccess) {
            vsc_set_error("%s: uploading %s failed", tag, name.c_str());
            return VSC_ERR_HIP;
        }
        return rc;
    }
    int upload_bf16(const std::string &name, int64_t rows, int cols, int cols_pad, uint16_t **out) {
        return upload_bf16(host_w.at(name), name, rows, cols, cols_pad, out);
    }

    // ---- the two lanes: consecutive max_batch chunks of one forward call alternate over two internal streams.  WHEN they are
    // made is the model's decision (ViT: finalize; Swin: the first call with more than one chunk) ----
    hipStream_t lane_stream[2] = {nullptr, nullptr};
    hipEvent_t ev_fork = nullptr, ev_join[2] = {nullptr, nullptr};
    bool lanes_ready = false;

    // idempotent per object: a call that failed part-way is resumed, not repeated
    int make_lanes() {
        if (lanes_ready) return VSC_OK;
        for (int l = 0; l < 2; ++l) {
            if (!lane_stream[l]) VSC_CHECK_HIP(hipStreamCreateWithFlags(&lane_stream[l], hipStreamNonBlocking));
            if (!ev_join[l]) VSC_CHECK_HIP(hipEventCreateWithFlags(&ev_join[l], hipEventDisableTiming));
        }
        if (!ev_fork) VSC_CHECK_HIP(hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming));
        lanes_ready = true;
        return VSC_OK;
    }
    int fork(hipStream_t user) {
        VSC_CHECK_HIP(hipEventRecord(ev_fork, user));
        for (int l = 0; l < 2; ++l) VSC_CHECK_HIP(hipStreamWaitEvent(lane_stream[l], ev_fork, 0));
        return VSC_OK;
    }
    // After the chunk loop, whatever it returned (rc): what the lanes already hold is ordered before the caller's next work on
    // `user`, so the caller may free or reuse frames / desc once its stream has drained.  Returns rc, or the first failed join.
    int join(hipStream_t user, int rc) {
        for (int l = 0; l < 2; ++l) {
            const hipError_t e1 = hipEventRecord(ev_join[l], lane_stream[l]);
            const hipError_t e2 = e1 == hipSuccess ? hipStreamWaitEvent(user, ev_join[l], 0) : e1;
            if (e2 != hipSuccess && !rc) {
                vsc_set_error("%sforward: joining lane %d failed: %s", api, l, hipGetErrorString(e2));
                rc = VSC_ERR_HIP;
            }
        }
        return rc;
    }

    // ---- optional per-launch timing: HIP events around every launch, summed per class.  While it is on, the chunks of a call
    // run back to back on the caller's stream (the events are meant to time one kernel at a time) ----
    static constexpr int MAX_CLASSES = 32;
    static constexpr size_t MAX_EVENTS = 1 << 16, BAD = ~(size_t)0;
    struct Span { int cls; size_t e0, e1; };
    bool profile = false;
    std::vector<hipEvent_t> ev_pool;
    size_t ev_used = 0;
    std::vector<Span> spans;
    double prof_ms[MAX_CLASSES] = {0};
    int64_t prof_n[MAX_CLASSES] = {0};

    // One event from the pool (recycled by collect / reset), recorded on st.  A failed create / record, or a pool that has grown
    // past MAX_EVENTS because nobody collects the profile, switches profiling off instead of recording garbage.
    size_t record(hipStream_t st) {
        if (ev_used == ev_pool.size()) {
            hipEvent_t ev;
            if (ev_pool.size() >= MAX_EVENTS || hipEventCreate(&ev) != hipSuccess) {
                profile = false;
                return BAD;
            }
            ev_pool.push_back(ev);
        }
        if (hipEventRecord(ev_pool[ev_used], st) != hipSuccess) {
            profile = false;
            return BAD;
        }
        return ev_used++;
    }
    void reset(bool on) {
        profile = on;
        spans.clear();
        ev_used = 0;
        for (int i = 0; i < MAX_CLASSES; ++i) {
            prof_ms[i] = 0;
            prof_n[i] = 0;
        }
    }
    int collect(double *ms_out, int64_t *n_out, int classes) {
        VSC_CHECK_HIP(hipDeviceSynchronize());
        for (const Span &sp : spans) {
            float ms = 0.f;
            VSC_CHECK_HIP(hipEventElapsedTime(&ms, ev_pool[sp.e0], ev_pool[sp.e1]));
            prof_ms[sp.cls] += ms;
            prof_n[sp.cls] += 1;
        }
        spans.clear();
        ev_used = 0;
        for (int i = 0; i < classes; ++i) {
            ms_out[i] = prof_ms[i];
            n_out[i] = prof_n[i];
        }
        return VSC_OK;
    }

    ~ModelHost() {
        for (void *p : allocs) (void)hipFree(p);
        for (hipEvent_t ev : ev_pool) (void)hipEventDestroy(ev);
        for (int l = 0; l < 2; ++l) {
            if (lane_stream[l]) (void)hipStreamDestroy(lane_stream[l]);
            if (ev_join[l]) (void)hipEventDestroy(ev_join[l]);
        }
        if (ev_fork) (void)hipEventDestroy(ev_fork);
    }
};

// times the launches of one scope on st under class cls while profiling is on
struct ProfScope {
    ModelHost *m;
    hipStream_t st;
    size_t e0 = 0;
    int cls;
    ProfScope(ModelHost *m_, int c, hipStream_t s) : m(m_), st(s), cls(c) {
        if (m->profile) e0 = m->record(st);
    }
    ~ProfScope() {
        if (!m->profile || e0 == ModelHost::BAD) return;
        const size_t e1 = m->record(st);
        if (e1 != ModelHost::BAD) m->spans.push_back({cls, e0, e1});
    }
};
