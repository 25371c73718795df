// Move-only owners of what the host code holds on the HIP runtime: device and pinned buffers, events, streams.  Host-only, no device code.
// None of them synchronises: a caller that frees what a stream may still be using waits for that stream itself, where it can be read.
// They release on whatever device is current, so their holder makes the right one current first (Engine::~Engine, rccl_comm.cpp).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <stdexcept>
#include <string>

namespace goicp {

inline void hip_check(hipError_t e, const char* what)
{
	if (e != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
}
#define HIPCHK(x) ::goicp::hip_check((x), #x)

// memory policies of Buf: allocate bytes (or throw), free
struct Device {
	static void* alloc(size_t bytes) { void* p = nullptr; HIPCHK(hipMalloc(&p, bytes)); return p; }
	static void free(void* p) { (void)hipFree(p); }
};
struct Pinned {
	static void* alloc(size_t bytes) { void* p = nullptr; HIPCHK(hipHostMalloc(&p, bytes)); return p; }
	static void free(void* p) { (void)hipHostFree(p); }
};

// n elements of T, uninitialised.  Converts to the raw pointer, so it is passed to a launch or copied into a descriptor like the pointer
// it replaces.  Zero elements allocate one: a temporary sized by an absent optional output is still a real pointer
template <class T, class Mem = Device> class Buf {
	T* p_ = nullptr;
	size_t n_ = 0;

public:
	Buf() = default;
	explicit Buf(size_t n) { alloc(n); }
	~Buf() { reset(); }
	Buf(Buf&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
	Buf& operator=(Buf&& o) noexcept
	{
		if (this != &o) { reset(); p_ = o.p_; n_ = o.n_; o.p_ = nullptr; o.n_ = 0; }
		return *this;
	}
	T* get() const { return p_; }
	operator T*() const { return p_; }
	T* operator->() const { return p_; }
	explicit operator bool() const { return p_ != nullptr; }
	size_t size() const { return n_; }
	void reset() { if (p_) Mem::free(p_); p_ = nullptr; n_ = 0; }
	// exactly n, whatever was held; empty when the allocation throws
	void alloc(size_t n) { reset(); p_ = static_cast<T*>(Mem::alloc(sizeof(T) * (n ? n : 1))); n_ = n; }
	// grow-only; true when it allocated anew: the pointer changed and the contents are gone
	bool reserve(size_t n) { if (n <= n_) return false; alloc(n); return true; }
};
template <class T> using PinnedBuf = Buf<T, Pinned>;

// an event or a stream: null until create()
template <class H, hipError_t (*Destroy)(H)> class Handle {
	H h_ = nullptr;

public:
	Handle() = default;
	~Handle() { reset(); }
	Handle(Handle&& o) noexcept : h_(o.h_) { o.h_ = nullptr; }
	Handle& operator=(Handle&& o) noexcept
	{
		if (this != &o) { reset(); h_ = o.h_; o.h_ = nullptr; }
		return *this;
	}
	operator H() const { return h_; }
	void reset() { if (h_) (void)Destroy(h_); h_ = nullptr; }

protected:
	H* fresh() { reset(); return &h_; }
};
struct Event : Handle<hipEvent_t, hipEventDestroy> {
	void create(unsigned flags = hipEventDefault) { HIPCHK(hipEventCreateWithFlags(fresh(), flags)); }   // hipEventDisableTiming: ordering only
};
struct Stream : Handle<hipStream_t, hipStreamDestroy> {   // non-blocking, as every stream of the library
	void create() { HIPCHK(hipStreamCreateWithFlags(fresh(), hipStreamNonBlocking)); }
	void create(int priority) { HIPCHK(hipStreamCreateWithPriority(fresh(), hipStreamNonBlocking, priority)); }
};

}  // namespace goicp
