// vr_staging.h -- the device buffers of ONE call of an entry point that takes its arrays on the
// host or on the device (vr_query_api.cpp, vr_scene.cpp).  Private, as vr_host.h.
#pragma once

#include <hip/hip_runtime.h>

#include <vector>

#pragma GCC visibility push(hidden)

namespace vr {

// What a call stages through `stream`: device copies of its host inputs, device scratch, device
// results on their way to the host.  The one rule it keeps: a buffer is freed when the call
// returns, on every path, and never while a copy or kernel that uses it may still be queued --
// unless the stream is known to have drained (sync(), drained()), the destructor waits for it
// first.  That wait happens on failure paths only: a call that succeeds has drained the stream.
// The first error sticks in `err` and turns every later operation into a no-op, so a caller
// checks once per stage.
struct Staging {
    const hipStream_t stream;
    hipError_t err = hipSuccess;

    explicit Staging(hipStream_t st) : stream(st) {}
    Staging(const Staging&) = delete;
    Staging& operator=(const Staging&) = delete;
    ~Staging() {
        if (!owned.empty() && busy) (void)hipStreamSynchronize(stream);
        for (void* p : owned) (void)hipFree(p);
    }

    // A device buffer for scratch or a result (null after an error).
    void* make(size_t bytes) {
        void* p = nullptr;
        if (err == hipSuccess) err = hipMalloc(&p, bytes);
        if (err != hipSuccess) return nullptr;
        owned.push_back(p);
        return p;
    }
    // A buffer another function allocated for this call (vr::trace_order's scratch; may be null).
    void adopt(void* p) {
        if (p) owned.push_back(p);
    }
    // Queue host -> dev; `dev` is, or lies in, a buffer of this call.
    void put(void* dev, const void* host, size_t bytes) {
        if (err == hipSuccess) err = hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, stream);
    }
    // The device copy of a host array.
    void* upload(const void* host, size_t bytes) {
        void* p = make(bytes);
        put(p, host, bytes);
        return err == hipSuccess ? p : nullptr;
    }
    // Queue dev -> host: a result's way back.  The host array is written once sync() returns.
    void fetch(void* host, const void* dev, size_t bytes) {
        if (err == hipSuccess) err = hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, stream);
    }
    // Wait for the stream (whatever `err` is: work of this call may be queued).
    hipError_t sync() {
        busy = false;
        return hipStreamSynchronize(stream);
    }
    // The caller knows the stream has drained since the last operation on a buffer of this call
    // (the device builders return after a hipStreamSynchronize of their own).
    void drained() { busy = false; }

private:
    std::vector<void*> owned;
    bool busy = true;
};

}  // namespace vr

#pragma GCC visibility pop
