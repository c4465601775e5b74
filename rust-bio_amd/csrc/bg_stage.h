// bg_stage: the device copies of a host-buffer entry point (bg_common.h includes this).  Every `bg_x(host arrays)` that is
// `bg_x_dev` between an upload and a download stages its arrays through one of these.
#ifndef BG_STAGE_H
#define BG_STAGE_H

// Owns every device allocation made through it and frees them when it goes out of scope, whichever way the entry point
// returns.  `rc` keeps the first failure (bg_last_error names the call); after one, up / out return null and down / sync do
// nothing, so a call site stages all its inputs and looks at rc once.  A null or empty source is allocated and not copied;
// nothing is allocated smaller than 16 bytes, so an empty column still has an address a *_dev call accepts.
struct bg_stage {
    hipStream_t st;
    int rc = BG_OK;
    std::vector<void*> owned;

    bg_stage(const bg_ctx* ctx, hipStream_t s) : st(s) { note(hipSetDevice(ctx->device), "hipSetDevice(ctx->device)"); }
    bg_stage(const bg_stage&) = delete;
    bg_stage& operator=(const bg_stage&) = delete;
    ~bg_stage() {
        for (void* p : owned) hipFree(p);
    }
    int note(hipError_t e, const char* call) {
        if (e != hipSuccess && rc == BG_OK) {
            bg_tls_error = std::string(call) + ": " + hipGetErrorString(e);
            rc = e == hipErrorOutOfMemory ? BG_ERR_OOM : BG_ERR_HIP;
        }
        return rc;
    }
    // n elements on the device, not initialised
    template <class T>
    T* out(size_t n) {
        void* p = nullptr;
        if (rc || note(hipMalloc(&p, n * sizeof(T) < 16 ? 16 : n * sizeof(T)), "bg_stage: hipMalloc")) return nullptr;
        owned.push_back(p);
        return (T*)p;
    }
    // ... holding src[0 .. n) once the stream gets there
    template <class T>
    T* up(const T* src, size_t n) {
        T* p = out<T>(n);
        if (p && src && n) note(hipMemcpyAsync(p, src, n * sizeof(T), hipMemcpyHostToDevice, st), "bg_stage: hipMemcpyAsync to the device");
        return p;
    }
    template <class T>
    void down(T* dst, const T* d_src, size_t n) {
        if (!rc && n) note(hipMemcpyAsync(dst, d_src, n * sizeof(T), hipMemcpyDeviceToHost, st), "bg_stage: hipMemcpyAsync to the host");
    }
    int sync() {
        if (!rc) note(hipStreamSynchronize(st), "bg_stage: hipStreamSynchronize");
        return rc;
    }
};

#endif
