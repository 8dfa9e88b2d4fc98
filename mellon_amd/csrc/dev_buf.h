// The one owner of a block from alloc.hip: move-only, empty by default, released by its destructor.  HOW a block goes back
// is chosen where the buffer is declared: DevBuf<T> waits device-wide first (mln_dfree, the guarantee hipFree gives),
// StreamBuf<T> relies on its user having drained the one stream the block was used on, PinnedBuf<T> is page-locked host memory.
#pragma once

hipError_t mln_dfree_synced(void* p);                // alloc.hip: mln_dfree without the device-wide wait
hipError_t mln_hmalloc(void** out, size_t bytes);    // alloc.hip: page-locked host blocks, cached by size
hipError_t mln_hfree(void* p);

struct FreeDevice { static hipError_t get(void** p, size_t b) { return mln_dmalloc(p, b); } static void put(void* p) { (void)mln_dfree(p); } };
struct FreeSynced { static hipError_t get(void** p, size_t b) { return mln_dmalloc(p, b); } static void put(void* p) { (void)mln_dfree_synced(p); } };
struct FreePinned { static hipError_t get(void** p, size_t b) { return mln_hmalloc(p, b); } static void put(void* p) { (void)mln_hfree(p); } };

template <class T, class Release = FreeDevice>
class DevBuf {
  T* p_ = nullptr;
 public:
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p_(o.p_) { o.p_ = nullptr; }
  DevBuf& operator=(DevBuf&& o) noexcept { if (this != &o) { reset(); p_ = o.p_; o.p_ = nullptr; } return *this; }
  ~DevBuf() { reset(); }
  int alloc(mln_ctx* ctx, size_t count, const char* what) {   // a buffer that holds a block releases it first
    reset();
    const hipError_t e = Release::get((void**)&p_, count * sizeof(T));
    if (e == hipSuccess) return MLN_OK;
    p_ = nullptr;
    return mln_hip_fail(ctx, e, what, __FILE__, __LINE__);
  }
  int alloc_zeroed(mln_ctx* ctx, size_t count, const char* what);   // + a memset enqueued on ctx->stream (mln_core.h, below mln_ctx)
  void reset() { if (p_) { Release::put(p_); p_ = nullptr; } }
  T* get() const { return p_; }
  operator T*() const { return p_; }
  T* operator->() const { return p_; }
  explicit operator bool() const { return p_ != nullptr; }
};
template <class T> using StreamBuf = DevBuf<T, FreeSynced>;
template <class T> using PinnedBuf = DevBuf<T, FreePinned>;
