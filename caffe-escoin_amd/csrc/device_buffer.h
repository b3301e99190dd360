// device_buffer.h -- owners of the library's device allocations: a plan's device bytes are what its owners hold.
#ifndef ESCOIN_DEVICE_BUFFER_H_
#define ESCOIN_DEVICE_BUFFER_H_

#include <hip/hip_runtime_api.h>

#include <utility>
#include <vector>

namespace escoin {

// One hipMalloc allocation, freed on destruction, by reset() and when another buffer is moved in.  Move-only.
class DeviceBuffer {
 public:
  DeviceBuffer() = default;
  DeviceBuffer(DeviceBuffer &&o) noexcept { *this = std::move(o); }
  DeviceBuffer &operator=(DeviceBuffer &&o) noexcept {
    if (this != &o) reset(), std::swap(ptr_, o.ptr_), std::swap(bytes_, o.bytes_);
    return *this;
  }
  ~DeviceBuffer() { reset(); }
  // frees what the buffer held, then allocates `bytes` (a failed allocation leaves the buffer empty)
  hipError_t alloc(size_t bytes) {
    reset();
    const hipError_t e = hipMalloc(&ptr_, bytes);
    if (e == hipSuccess) bytes_ = bytes;
    else ptr_ = nullptr;
    return e;
  }
  // alloc() for `src`, which is then copied in on `stream` (src must outlive the copy)
  template <typename T> hipError_t upload(const std::vector<T> &src, hipStream_t stream) {
    hipError_t e = alloc(sizeof(T) * src.size());
    if (e == hipSuccess) e = hipMemcpyAsync(ptr_, src.data(), bytes_, hipMemcpyHostToDevice, stream);
    return e;
  }
  void reset() {
    if (ptr_) (void)hipFree(ptr_);
    ptr_ = nullptr;
    bytes_ = 0;
  }
  size_t bytes() const { return bytes_; }
  template <typename T> T *get() const { return static_cast<T *>(ptr_); }

 private:
  void *ptr_ = nullptr;
  size_t bytes_ = 0;
};

// One word of pinned host memory the device writes through (hipHostMallocMapped) and its device address, owned like a
// DeviceBuffer (host memory: not among a plan's device bytes).
class MappedWord {
 public:
  MappedWord() = default;
  MappedWord(MappedWord &&o) noexcept { *this = std::move(o); }
  MappedWord &operator=(MappedWord &&o) noexcept {
    if (this != &o) reset(), std::swap(host_, o.host_), std::swap(dev_, o.dev_);
    return *this;
  }
  ~MappedWord() { reset(); }
  // frees what it held, then allocates the word, zeroed, and looks up its device address
  hipError_t alloc() {
    reset();
    const hipError_t e = hipHostMalloc((void **)&host_, 64, hipHostMallocMapped);
    if (e != hipSuccess) return host_ = nullptr, e;
    *host_ = 0u;
    return hipHostGetDevicePointer((void **)&dev_, host_, 0);
  }
  void reset() {
    if (host_) (void)hipHostFree(host_);
    host_ = dev_ = nullptr;
  }
  unsigned *host() const { return host_; }
  unsigned *device() const { return dev_; }

 private:
  unsigned *host_ = nullptr, *dev_ = nullptr;
};

}  // namespace escoin
#endif
