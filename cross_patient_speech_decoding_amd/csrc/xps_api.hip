// Error reporting, ABI version and run-time switch table of libxps.so.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <atomic>
#include "xps_common.h"
#include "xps_switches.h"

static thread_local char g_err[512] = "";

void xps_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

extern "C" const char* xps_last_error(void) { return g_err; }
// 2: round 2 (xps_gru_seq_fwd_f32 takes a workspace; fused-dropout, decoder-select, big-tile and augmentation entry points added)
extern "C" int xps_abi_version(void) { return 4; }

// ---- the switch table (xps_switches.h) ----
namespace {
using xps_sw::COUNT;
long long on_unless_0(const char* e, long long) { return e[0] == '0' ? 0 : 1; }
long long off_unless_1(const char* e, long long) { return e[0] == '1' ? 1 : 0; }
long long int_at_least_0(const char* e, long long def) { const int v = atoi(e); return v >= 0 ? v : def; }
long long int_above_0(const char* e, long long def) { const int v = atoi(e); return v > 0 ? v : def; }
long long precision_name(const char* e, long long def) { return (!strcmp(e, "fp32") || !strcmp(e, "f32") || !strcmp(e, "0")) ? 0 : ((!strcmp(e, "bf16x3") || !strcmp(e, "1")) ? 1 : def); }
long long cluster_name(const char* e, long long def) { return (!strcmp(e, "off") || !strcmp(e, "0")) ? 0 : ((!strcmp(e, "steps") || !strcmp(e, "1")) ? 1 : def); }
long long reduce_name(const char* e, long long) { return e[0] == 'f' ? 1 : (e[0] == 'l' ? 2 : 0); }

struct SwitchRow {
    const char* name;
    long long def, lo, hi;                                  // xps_set_switch takes lo <= value <= hi
    long long (*parse)(const char* text, long long def);    // the environment's text (never null) -> value
};
constexpr long long BOOL = 1, ANY = 0x7fffffff;
const SwitchRow g_rows[COUNT] = {                           // in the order of xps_sw::Id
    {"XPS_GEMM_PRECISION", 1, 0, 1, precision_name},
    {"XPS_GEMM_SMALL_TILE_BLOCKS", 2048, 0, ANY, int_at_least_0},
    {"XPS_GEMM_LONGK_128", 1, 0, BOOL, on_unless_0},
    {"XPS_GEMM_BIG", 1, 0, BOOL, on_unless_0},
    {"XPS_GEMM_DMA", 1, 0, BOOL, on_unless_0},
    {"XPS_PROJ_WS", 1, 0, BOOL, on_unless_0},
    {"XPS_GEMM_BIG_DEEP", 0, 0, BOOL, off_unless_1},
    {"XPS_GEMM_BIG_MIN_TILES", 192, 1, ANY, int_above_0},
    {"XPS_GEMM_BIG_TAIL", 1, 0, BOOL, on_unless_0},
    {"XPS_TN_BLOCKS", 512, 1, ANY, int_above_0},
    {"XPS_TN_UNIFORM", 0, 0, BOOL, off_unless_1},
    {"XPS_GEMM_BIG_DEEP_TN", 0, 0, BOOL, off_unless_1},
    {"XPS_TN_REDUCE", 0, 0, 2, reduce_name},
    {"XPS_GRU_STEP_PATH", 1, 0, BOOL, on_unless_0},
    {"XPS_GRU_CLUSTER", 2, 0, 2, cluster_name},
    {"XPS_GRU_CL_CUS", 0, 0, ANY, int_at_least_0},          // (0 and below: no cap)
    {"XPS_GRU_CL2", 0, 0, BOOL, off_unless_1},
    {"XPS_GRU_XIMG", 1, 0, BOOL, on_unless_0},
    {"XPS_GRU_XOUT", 0, 0, BOOL, off_unless_1},
};

std::atomic<long long>* switch_values() {
    static std::atomic<long long> v[COUNT];
    static const bool filled = [] {
        for (int i = 0; i < COUNT; ++i) {
            const char* e = getenv(g_rows[i].name);
            v[i].store(e ? g_rows[i].parse(e, g_rows[i].def) : g_rows[i].def, std::memory_order_relaxed);
        }
        return true;
    }();
    (void)filled;
    return v;
}
int switch_id(const char* name) {
    for (int i = 0; name && i < COUNT; ++i)
        if (!strcmp(name, g_rows[i].name)) return i;
    return -1;
}
}  // namespace

long long xps_sw::get(Id id) { return switch_values()[id].load(std::memory_order_relaxed); }
void xps_sw::store(Id id, long long value) { switch_values()[id].store(value, std::memory_order_relaxed); }

extern "C" int xps_set_switch(const char* name, long long value) {
    const int i = switch_id(name);
    if (i < 0) { xps_set_error("xps_set_switch: no switch named %s (xps_list_switches names them)", name ? name : "(null)"); return XPS_E_INVALID; }
    if (value < g_rows[i].lo || value > g_rows[i].hi) {
        xps_set_error("xps_set_switch: %s takes %lld .. %lld, not %lld", name, g_rows[i].lo, g_rows[i].hi, value);
        return XPS_E_INVALID;
    }
    xps_sw::store((xps_sw::Id)i, value);
    return XPS_OK;
}

extern "C" int xps_get_switch(const char* name, long long* value) {
    const int i = switch_id(name);
    if (i < 0 || !value) { xps_set_error("xps_get_switch: %s", i < 0 ? "no switch of that name" : "null argument"); return XPS_E_INVALID; }
    *value = xps_sw::get((xps_sw::Id)i);
    return XPS_OK;
}

extern "C" int xps_list_switches(char* buf, size_t n) {
    if (!buf || n == 0) { xps_set_error("xps_list_switches: no buffer"); return XPS_E_INVALID; }
    size_t used = 0;
    buf[0] = 0;
    for (int i = 0; i < COUNT; ++i) {
        const int w = snprintf(buf + used, n - used, "%s=%lld\n", g_rows[i].name, xps_sw::get((xps_sw::Id)i));
        if (w < 0 || (size_t)w >= n - used) { xps_set_error("xps_list_switches: the buffer of %zu bytes is too small", n); return XPS_E_INVALID; }
        used += (size_t)w;
    }
    return XPS_OK;
}

// A stream at the LOWEST priority the device offers (torch exposes only "default" and "high"): the side stream
// of the weight-gradient GEMMs must never be preferred over the critical path when a CU frees up.
extern "C" int xps_stream_create_low_priority(void** stream) {
    if (!stream) { xps_set_error("xps_stream_create_low_priority: null argument"); return XPS_E_INVALID; }
    int least = 0, greatest = 0;
    if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) { least = 0; }
    hipStream_t s = nullptr;
    if (hipStreamCreateWithPriority(&s, hipStreamNonBlocking, least) != hipSuccess) {
        xps_set_error("xps_stream_create_low_priority: hipStreamCreateWithPriority failed");
        return XPS_E_HIP;
    }
    *stream = (void*)s;
    return XPS_OK;
}

extern "C" int xps_stream_destroy(void* stream) {
    if (stream && hipStreamDestroy((hipStream_t)stream) != hipSuccess) return XPS_E_HIP;
    return XPS_OK;
}
