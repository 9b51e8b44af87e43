// The owner of one hipMalloc block: every device table, key and temporary of the library is an lm_dev, and this is the
// one place where the library spells hipFree -- set storage (the context's pool, lm_ctx.hip) and the candidate blocks of
// the scratch placement (lm_ks_scratch.hip) aside.  DESIGN.md, "Who owns device memory".
#pragma once
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/lumenos_hip.h"

int lm_fail(lumen_ctx *ctx, const char *fmt, ...);

// The fill-and-fence mode (LUMEN_ALLOC_FILL; lm_ctx.hip; DESIGN.md, "Who owns device memory").  Off, a block is drawn and
// freed exactly as without it.  On, a block is drawn with LM_GUARD_BYTES behind it, filled with the byte before its first
// use, the band with a canary; the band is read back when the block goes (and by lumen_ctx_alloc_check).
#define LM_GUARD_BYTES ((size_t)4096)
// the fill byte `ctx` draws under (NULL: what lumen_ctx_create last read from the environment); 0 = the mode is off
unsigned lm_alloc_fill_byte(const lumen_ctx *ctx);
// fills [p, p + bytes) with the byte and -- band -- the LM_GUARD_BYTES behind it with the canary, on the context's
// stream (NULL: blocking), and waits; returns the canary, 0 after an error (reported through lm_fail)
unsigned char lm_alloc_fill(lumen_ctx *ctx, void *p, size_t bytes, unsigned fill, bool band, const char *what);
// reads the band behind [p, p + bytes) back (a blocking copy): 0, or 1 with the first changed byte reported -- through
// lm_fail(ctx, ...), which prints it on stderr
int lm_alloc_band_check(lumen_ctx *ctx, const void *p, size_t bytes, unsigned char canary, const char *what);

template <class T>
class lm_dev {
    T *p_ = nullptr;
    size_t n_ = 0;
    hipStream_t stream_ = nullptr; // release_on
    bool wipe_ = false;
    unsigned char canary_ = 0; // of the guard band behind the block; 0: none (the mode was off, or a block drawn elsewhere)
    char what_[40] = {0};      // a guarded block's name, for the report

    size_t bytes_() const { return (n_ ? n_ : 1) * sizeof(T); }
    void take_guard(const lm_dev &o) {
        canary_ = o.canary_;
        memcpy(what_, o.what_, sizeof(what_));
    }

  public:
    lm_dev() = default;
    lm_dev(T *block, size_t count) : p_(block), n_(count) {} // takes over a block drawn elsewhere (a placement's choice)
    lm_dev(lm_dev &&o) noexcept : p_(o.release()), n_(o.n_), stream_(o.stream_), wipe_(o.wipe_) { take_guard(o); }
    lm_dev &operator=(lm_dev &&o) noexcept {
        if (this != &o) {
            reset();
            n_ = o.n_, stream_ = o.stream_, wipe_ = o.wipe_;
            take_guard(o);
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
        const unsigned fill = lm_alloc_fill_byte(ctx);
        if (hipMalloc((void **)&p_, bytes + (fill ? LM_GUARD_BYTES : 0)) != hipSuccess) {
            (void)hipGetLastError();
            p_ = nullptr;
            return lm_fail(ctx, "hipMalloc(%zu bytes) for %s failed", bytes, what);
        }
        n_ = count, canary_ = 0;
        if (fill) {
            snprintf(what_, sizeof(what_), "%s", what);
            if (!(canary_ = lm_alloc_fill(ctx, p_, bytes, fill, true, what))) {
                reset();
                return 1;
            }
        }
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
    // the guard band's canary (0: the block has none) and the name the block was drawn under
    unsigned char canary() const { return canary_; }
    const char *what() const { return what_; }
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
        if (canary_) (void)lm_alloc_band_check(nullptr, p_, bytes_(), canary_, what_);
        canary_ = 0;
        (void)hipFree(release());
        (void)hipGetLastError();
    }
};
