// The two owners of what the host side allocates: DeviceBuffer<T> (hipMalloc) and PinnedBuffer<T> (hipHostMalloc with the
// caller's flags), each with its element count.  Move-only; the destructor frees.  They report nothing, wait for nothing and do not
// choose the device: the caller has made the context's device current and drained what may still use the memory, and words a
// failed alloc() into its own refusal.  Kernel argument structs hold raw pointers filled from get(); an owner is never passed
// to a launch.
#pragma once
#include <hip/hip_runtime.h>

#include <utility>

namespace kws {

template <class T>
class DeviceBuffer {
  public:
    DeviceBuffer() = default;
    DeviceBuffer(DeviceBuffer&& o) noexcept : p_(std::exchange(o.p_, nullptr)), n_(std::exchange(o.n_, 0)) {}
    DeviceBuffer& operator=(DeviceBuffer&& o) noexcept {  // frees what it held, takes what o holds
        if (this != &o) {
            reset();
            p_ = std::exchange(o.p_, nullptr);
            n_ = std::exchange(o.n_, 0);
        }
        return *this;
    }
    ~DeviceBuffer() { reset(); }
    bool alloc(size_t n) {  // n elements, contents undefined; frees what it held first.  false: nothing is held
        reset();
        if (hipMalloc(reinterpret_cast<void**>(&p_), n * sizeof(T)) != hipSuccess) p_ = nullptr;
        n_ = p_ ? n : 0;
        return p_ != nullptr;
    }
    void reset() {
        if (p_) (void)hipFree(p_);
        p_ = nullptr, n_ = 0;
    }
    T* get() const { return p_; }
    size_t size() const { return n_; }
    explicit operator bool() const { return p_ != nullptr; }

  private:
    T* p_ = nullptr;
    size_t n_ = 0;
};

template <class T>
class PinnedBuffer {
  public:
    PinnedBuffer() = default;
    PinnedBuffer(PinnedBuffer&& o) noexcept : p_(std::exchange(o.p_, nullptr)), n_(std::exchange(o.n_, 0)) {}
    PinnedBuffer& operator=(PinnedBuffer&& o) noexcept {
        if (this != &o) {
            reset();
            p_ = std::exchange(o.p_, nullptr);
            n_ = std::exchange(o.n_, 0);
        }
        return *this;
    }
    ~PinnedBuffer() { reset(); }
    bool alloc(size_t n, unsigned flags) {  // n elements pinned with `flags` (hipHostMalloc*); otherwise as DeviceBuffer::alloc
        reset();
        if (hipHostMalloc(reinterpret_cast<void**>(&p_), n * sizeof(T), flags) != hipSuccess) p_ = nullptr;
        n_ = p_ ? n : 0;
        return p_ != nullptr;
    }
    void reset() {
        if (p_) (void)hipHostFree(p_);
        p_ = nullptr, n_ = 0;
    }
    T* get() const { return p_; }
    size_t size() const { return n_; }
    explicit operator bool() const { return p_ != nullptr; }

  private:
    T* p_ = nullptr;
    size_t n_ = 0;
};

}  // namespace kws
