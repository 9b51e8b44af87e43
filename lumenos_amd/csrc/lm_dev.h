// The owner of one hipMalloc block: every device table, key and temporary of the library is an lm_dev, and this is the
// one place where the library spells hipFree -- set storage (the context's pool, lm_ctx.hip) and the candidate blocks of
// the scratch placement (lm_ks_scratch.hip) aside.  DESIGN.md, "Who owns device memory".
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "../../include/lumenos_hip.h"

int lm_fail(lumen_ctx *ctx, const char *fmt, ...);

template <class T>
class lm_dev {
    T *p_ = nullptr;
    size_t n_ = 0;
    hipStream_t stream_ = nullptr; // release_on
    bool wipe_ = false;

  public:
    lm_dev() = default;
    lm_dev(T *block, size_t count) : p_(block), n_(count) {} // takes over a block drawn elsewhere (a placement's choice)
    lm_dev(lm_dev &&o) noexcept : p_(o.release()), n_(o.n_), stream_(o.stream_), wipe_(o.wipe_) {}
    lm_dev &operator=(lm_dev &&o) noexcept {
        if (this != &o) {
            reset();
            n_ = o.n_, stream_ = o.stream_, wipe_ = o.wipe_;
            p_ = o.release();
        }
        return *this;
    }
    lm_dev(const lm_dev &) = delete;
    lm_dev &operator=(const lm_dev &) = delete;
    ~lm_dev() { reset(); }

    // What precedes the free.  A temporary that kernels on `s` use: wait for `s`.  wipe (secrets: s, its images, the
    // errors): zero the block first -- enqueued on `s` and waited for, or with a blocking hipMemset when `s` is NULL.
    lm_dev &release_on(hipStream_t s, bool wipe) {
        stream_ = s, wipe_ = wipe;
        return *this;
    }
    // frees what it held; count == 0 still draws one element (callers rely on a non-NULL pointer)
    int alloc(lumen_ctx *ctx, size_t count, const char *what) {
        reset();
        const size_t bytes = (count ? count : 1) * sizeof(T);
        if (hipMalloc((void **)&p_, bytes) != hipSuccess) {
            (void)hipGetLastError();
            p_ = nullptr;
            return lm_fail(ctx, "hipMalloc(%zu bytes) for %s failed", bytes, what);
        }
        n_ = count;
        return 0;
    }
    // alloc + a blocking copy: one-off table loads out of pageable memory
    int upload(lumen_ctx *ctx, const T *host, size_t count, const char *what) {
        if (int rc = alloc(ctx, count, what)) return rc;
        if (count && hipMemcpy(p_, host, count * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) {
            (void)hipGetLastError();
            reset();
            return lm_fail(ctx, "hipMemcpy(%zu bytes) to the device for %s failed", count * sizeof(T), what);
        }
        return 0;
    }
    int upload(lumen_ctx *ctx, const std::vector<T> &host, const char *what) { return upload(ctx, host.data(), host.size(), what); }

    T *get() const { return p_; }
    size_t count() const { return n_; }
    explicit operator bool() const { return p_ != nullptr; }
    T *release() {
        T *r = p_;
        p_ = nullptr;
        return r;
    }
    void reset() {
        if (!p_) return;
        if (wipe_) (void)(stream_ ? hipMemsetAsync(p_, 0, n_ * sizeof(T), stream_) : hipMemset(p_, 0, n_ * sizeof(T)));
        if (stream_) (void)hipStreamSynchronize(stream_);
        (void)hipFree(release());
        (void)hipGetLastError();
    }
};
