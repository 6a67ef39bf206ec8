// finenv_host.h -- host-side helpers shared by the C-ABI entry points.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <new>

#include "finenv.h"

namespace finenv_host {

// HIP device that owns a device pointer, or -1 (host pointer, no device, unknown).
inline int pointer_device(const void *p)
{
    hipPointerAttribute_t a;
    if (p != nullptr && hipPointerGetAttributes(&a, p) == hipSuccess &&
        a.type == hipMemoryTypeDevice)
        return a.device;
    (void)hipGetLastError();
    return -1;
}

// Launches go to the device that owns the handle's state block, whatever the calling thread's
// current device is (a caller holding tensors on cuda:3 without a set_device would otherwise
// launch on device 0 with device-3 pointers).  Restores the previous device on scope exit.
struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int want)
    {
        int cur = -1;
        if (want >= 0 && hipGetDevice(&cur) == hipSuccess && cur != want &&
            hipSetDevice(want) == hipSuccess)
            prev = cur;
    }
    ~DeviceGuard()
    {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
    DeviceGuard(const DeviceGuard &) = delete;
    DeviceGuard &operator=(const DeviceGuard &) = delete;
};

// The part every env handle shares: each struct finenv_<kind> derives from it and adds its own
// cfg / panel / st and whatever else is its own.
struct Handle {
    int device;           // HIP device that owns the bound state block (-1 before bind)
    int bound;
    int D;                // observation width (floats)
    char err[256];        // finenv_<kind>_last_error
};

inline int fail(Handle *h, int code, const char *msg)
{
    if (h) snprintf(h->err, sizeof(h->err), "%s", msg);
    return code;
}

inline int check_launch(Handle *h, const char *what)
{
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        snprintf(h->err, sizeof(h->err), "%s: %s", what, hipGetErrorString(e));
        return FINENV_ERR_HIP;
    }
    return FINENV_OK;
}

// Ready to launch: a null handle is FINENV_ERR_INVALID, an unbound one FINENV_ERR_UNBOUND with
// "<what>: bind first".  The caller then takes a DeviceGuard(h->device).
inline int ready(Handle *h, const char *what)
{
    if (!h) return FINENV_ERR_INVALID;
    if (!h->bound) {
        snprintf(h->err, sizeof(h->err), "%s: bind first", what);
        return FINENV_ERR_UNBOUND;
    }
    return FINENV_OK;
}

// ready() for an entry point that works on an optional block of a non-null handle: a block that is not
// attached is FINENV_ERR_INVALID with "<what>: <missing>", and that is checked before the binding.
inline int ready_block(Handle *h, bool attached, const char *what, const char *missing)
{
    if (attached) return ready(h, what);
    snprintf(h->err, sizeof(h->err), "%s: %s", what, missing);
    return FINENV_ERR_INVALID;
}

// The two optional blocks of an env handle (members `has_hist`, and `last` where the kind has one): null
// handle, then ready_block().
template <class H>
int ready_history(H *h, const char *what)
{
    return h ? ready_block(h, h->has_hist != 0, what, "no history attached") : FINENV_ERR_INVALID;
}

template <class H>
int ready_last_episode(H *h, const char *what)
{
    return h ? ready_block(h, h->last != nullptr, what, "no last-episode block set") : FINENV_ERR_INVALID;
}

// finenv_<kind>_set_history behind the handle check: NULL detaches and zeroes the stored struct.
// `missing` is the kind's complaint about its own mandatory pointers (nullptr: all there); a refused
// struct leaves the attached one as it was.  min_capacity: 2 where arming writes entry 0, 1 where an
// armed record is empty.
template <class Hist>
int set_history(Handle *h, Hist &stored, int &has_hist, const Hist *hist, const char *missing,
                int min_capacity = 2)
{
    if (!hist) {
        has_hist = 0;
        memset(&stored, 0, sizeof(stored));
        return FINENV_OK;
    }
    if (missing) return fail(h, FINENV_ERR_INVALID, missing);
    if (hist->capacity < min_capacity) {
        if (h) snprintf(h->err, sizeof(h->err), "set_history: capacity must be >= %d", min_capacity);
        return FINENV_ERR_INVALID;
    }
    stored = *hist;
    has_hist = 1;
    return FINENV_OK;
}

// finenv_<kind>_history_arm: `launch(h, mask, stream)` is the kind's own arm kernel, `what` the label of
// a failed launch.
template <class H, class Launch>
int history_arm(H *h, const uint8_t *mask, void *stream, const char *what, Launch launch)
{
    if (const int rc = ready_history(h, "history_arm")) return rc;
    const DeviceGuard guard(h->device);
    launch(h, mask, (hipStream_t)stream);
    return check_launch(h, what);
}

// The series finenv_<kind>_history_metrics reads, and the argument of the one kernel that does
// (finenv_history.hip).  Every column is time-major, entry k of env e at [k * E + e].
struct HistorySeries {
    const double *value;          // the account value [capacity][E]
    const double *plus;           // added to `value` entry by entry, or NULL (two-wave: cash + asset_value)
    const double *ret;            // the recorded returns, read from entry 0, or NULL: total(k) / total(k-1) - 1
                                  // from entry 1.  `plus` is ignored when `ret` is set (no kind has both).
    const int32_t *len, *flags;   // [E]
    int32_t need;                 // FINENV_HIST_* bits a row must carry to count (0: `flags` is not read)
    int32_t capacity, E;
    double annualization;
    double *out;                  // [E][FINENV_STOCK_HISTORY_METRICS]
};

void launch_history_metrics(const HistorySeries &s, hipStream_t stream);

// finenv_<kind>_history_metrics: `series(h)` names the kind's columns (need, capacity and E with them).
template <class H, class Series>
int history_metrics(H *h, double annualization, double *out, void *stream, const char *what, Series series)
{
    if (!h || !out) return FINENV_ERR_INVALID;
    if (const int rc = ready_history(h, "history_metrics")) return rc;
    const DeviceGuard guard(h->device);
    HistorySeries s = series(h);
    s.annualization = annualization;
    s.out = out;
    launch_history_metrics(s, (hipStream_t)stream);
    return check_launch(h, what);
}

inline const char *last_error(const Handle *h) { return h ? h->err : "null handle"; }
inline int obs_dim(const Handle *h) { return h ? h->D : FINENV_ERR_INVALID; }

// A zeroed handle on no device with its config and observation width; nullptr when out of memory.
template <class H>
H *new_handle(const decltype(H::cfg) *cfg, long long D)
{
    H *h = new (std::nothrow) H();
    if (h) {
        h->device = -1;
        h->cfg = *cfg;
        h->D = (int)D;
    }
    return h;
}

// The end of every bind, once the pointers are checked: keep them, launch on the state's device.
template <class H>
int bind(H *h, const decltype(H::panel) *panel, const decltype(H::st) *st)
{
    h->panel = *panel;
    h->st = *st;
    h->device = pointer_device(st->f64);
    h->bound = 1;
    return FINENV_OK;
}

// magicN-style reciprocal: ceil(2^32 / n) for n >= 2 (exact f / n for f < 2^16), 0 for n < 2.
inline uint32_t magic_for(long long n)
{
    return n >= 2 ? (uint32_t)(((1ull << 32) + n - 1) / (unsigned long long)n) : 0u;
}

}  // namespace finenv_host
