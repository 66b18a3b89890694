// device_buffer.h — the one owner of a device or pinned-host allocation (plain C++17, no HIP types: the CPU suite tests
// it with a counting policy). Mem is a policy with static void* alloc(size_t bytes) (nullptr on failure) and
// void free(void*); the real ones (hipMalloc / hipHostMalloc, bgs_context.h) also clear HIP's sticky error on failure.
// Not a container: growing discards the contents.
#pragma once
#include <stddef.h>

namespace bgs {

template <class T, class Mem>
struct Buffer {
    T* ptr = nullptr;
    size_t capacity = 0;   // elements asked for (the allocation may be longer: reserve's min_bytes)

    Buffer() = default;
    Buffer(const Buffer&) = delete;
    Buffer& operator=(const Buffer&) = delete;
    Buffer(Buffer&& o) noexcept : ptr(o.ptr), capacity(o.capacity) { o.ptr = nullptr; o.capacity = 0; }
    Buffer& operator=(Buffer&& o) noexcept {
        if (this != &o) { reset(); ptr = o.ptr; capacity = o.capacity; o.ptr = nullptr; o.capacity = 0; }
        return *this;
    }
    ~Buffer() { reset(); }

    void reset() {
        if (ptr) Mem::free(ptr);
        ptr = nullptr;
        capacity = 0;
    }
    bool holds(size_t count) const { return ptr && count <= capacity; }
    // Room for `count` elements, and at least `min_bytes` bytes (a zero-length request still yields a live pointer). Keeps
    // what it has when that is enough; else frees FIRST (Mem::free waits for the device: nothing in flight still uses the
    // old allocation, and the two never coexist), then allocates. false: the buffer is empty ({nullptr, 0}).
    bool reserve(size_t count, size_t min_bytes = sizeof(T)) {
        if (holds(count)) return true;
        reset();
        const size_t bytes = count * sizeof(T);
        ptr = static_cast<T*>(Mem::alloc(bytes > min_bytes ? bytes : min_bytes));
        if (!ptr) return false;
        capacity = count;
        return true;
    }
    T* release() {   // hands the allocation to the caller
        T* p = ptr;
        ptr = nullptr;
        capacity = 0;
        return p;
    }
};

// Buffers that are only valid together (the sort's ping-pong lists and their culled tail, ...): all of them hold `count`
// elements afterwards (-1), or — an allocation failed — all of them are empty, so that the next call starts over, and the
// index of the member that could not be had is returned. All are freed before the first is allocated.
template <class... B>
int reserve_group(size_t count, B&... b) {
    if ((b.holds(count) && ...)) return -1;
    (b.reset(), ...);
    int got = 0;
    if (((b.reserve(count) && ++got) && ...)) return -1;
    (b.reset(), ...);
    return got;
}

}  // namespace bgs
