/* An owning device buffer: {pointer, bytes}, freed in the destructor.
 *
 * This header names the HIP runtime only through hipMalloc, hipFree,
 * hipMemcpy, hipMemset, hipSuccess and hipMemcpyHostToDevice, and does not
 * include the runtime header itself: the including file does that first
 * (tests/test_dev_buf_cpu.py compiles it against host stand-ins instead).
 *
 * hipFree is the synchronous one on purpose. A buffer may grow while
 * earlier work on the caller's stream still reads the old allocation, and
 * hipFree's implicit device synchronisation is what makes that safe. */
#ifndef FSDR_DEV_BUF_H
#define FSDR_DEV_BUF_H

#include <cstddef>

struct dev_buf {
    using status = decltype(hipSuccess);

    void* ptr = nullptr;
    size_t bytes = 0;

    dev_buf() = default;
    dev_buf(const dev_buf&) = delete;
    dev_buf& operator=(const dev_buf&) = delete;
    dev_buf(dev_buf&& o) noexcept : ptr(o.ptr), bytes(o.bytes) {
        o.ptr = nullptr;
        o.bytes = 0;
    }
    dev_buf& operator=(dev_buf&& o) noexcept {
        if (this != &o) {
            release();
            ptr = o.ptr;
            bytes = o.bytes;
            o.ptr = nullptr;
            o.bytes = 0;
        }
        return *this;
    }
    ~dev_buf() { release(); }

    void release() {
        if (ptr) (void)hipFree(ptr);
        ptr = nullptr;
        bytes = 0;
    }

    /* At least `want` bytes. Never shrinks; growth frees first, then
     * allocates (the contents are not kept), and a failed allocation
     * leaves {nullptr, 0}. */
    status ensure(size_t want) {
        if (bytes >= want) return hipSuccess;
        release();
        status e = hipMalloc(&ptr, want);
        if (e != hipSuccess) {
            ptr = nullptr;
            return e;
        }
        bytes = want;
        return hipSuccess;
    }

    /* Exactly n items of T, copied synchronously from the host; nothing
     * is left allocated if either step fails. */
    template <class T>
    status upload(const T* host, size_t n) {
        release();
        status e = hipMalloc(&ptr, n * sizeof(T));
        if (e != hipSuccess) {
            ptr = nullptr;
            return e;
        }
        bytes = n * sizeof(T);
        e = hipMemcpy(ptr, host, bytes, hipMemcpyHostToDevice);
        if (e != hipSuccess) release();
        return e;
    }

    status zero() { return hipMemset(ptr, 0, bytes); }

    template <class T>
    T* as() const { return static_cast<T*>(ptr); }
    explicit operator bool() const { return ptr != nullptr; }
};

#endif
