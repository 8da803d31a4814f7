// DevBuf: the owner of one block of the caching device allocator.  Nothing of HIP is needed here: a plain host compiler
// builds and tests the type (tests/c/devbuf_main.cpp) against its own dev_alloc / dev_free.
#pragma once
#include <cstddef>

namespace abz {

// caching device allocator (api.cpp): blocks freed with dev_free are reused by later dev_alloc calls.  dev_free files the
// block under the CURRENT device: whoever lets a DevBuf go (a destructor included) has selected the owner's device first.
int dev_alloc(void** out, size_t bytes, size_t* cap_out);
void dev_free(void* p, size_t cap);

// Move-only; the block goes back to the allocator with its owner.  A view points into a block owned elsewhere and is only
// forgotten.
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;     // of the block as the allocator handed it out (0 for a view)
    bool view = false;

    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap), view(o.view) { o.forget(); }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            release();
            p = o.p;
            cap = o.cap;
            view = o.view;
            o.forget();
        }
        return *this;
    }
    ~DevBuf() { release(); }

    static DevBuf view_of(void* q) {
        DevBuf b;
        b.p = q;
        b.view = true;
        return b;
    }
    // scratch that grows but never shrinks: nothing happens while bytes <= cap, else a block with room to spare
    int reserve(size_t bytes) {
        if (!view && bytes <= cap) return 0;
        int rc = alloc(bytes + (bytes >> 2) + 256);  // grow geometrically
        if (rc) rc = alloc(bytes);
        return rc;
    }
    // a fresh block of exactly `bytes` (rule values, tables, coefficients: what lives long is not over-allocated)
    int alloc(size_t bytes) {
        release();
        int rc = dev_alloc(&p, bytes, &cap);
        if (rc) forget();
        return rc;
    }
    void release() {
        if (!view) dev_free(p, cap);
        forget();
    }
    template <class T>
    T* as() const { return static_cast<T*>(p); }

private:
    void forget() {
        p = nullptr;
        cap = 0;
        view = false;
    }
};

}  // namespace abz
