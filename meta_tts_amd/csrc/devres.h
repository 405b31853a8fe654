// What a handle owns on the device, once: the check macro of every host-side runtime call, the allocator that remembers what it
// handed out (DevHeap), the grow-on-demand buffer on top of it (DevBuf / grow), and a side stream with its events (Lane).
//
// Every handle class (Engine, WaveGen — the base of Vocoder and HifiGan, wavegen.h —, DVector, MosNet, MelFront and what builds on it;
// the networks' weights sit in a ParamTable, params.h, allocated from it) holds ONE DevHeap and asks it for device memory,
// pinned host memory and single-purpose events; nothing else in this directory calls the runtime's allocation, stream-creation or
// event-creation entry points.  The heap frees whatever is left when it is told to (release_all) and when it dies, so a create that
// fails half way, a later reservation that fails, and destroy all end in the same place and free each block exactly once.  All of it
// is host-side bookkeeping at allocation time; nothing here sits on a per-launch path.
#pragma once
#include <algorithm>
#include <string>
#include <vector>

#include "compat.h"

namespace mtts {

// For member functions of a class with `int err(const std::string&)` (stores the message, returns -1).
#define DEV_CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return err(std::string(#x) + ": " + hipGetErrorString(e_)); } while (0)

class DevHeap {
    struct Block { void* p; bool pinned; };
    std::vector<Block> blocks;
    std::vector<hipEvent_t> events;
    hipError_t take(void** out, size_t bytes, bool pinned) {
        void* q = nullptr;
        const hipError_t e = pinned ? hipHostMalloc(&q, bytes) : hipMalloc(&q, bytes);
        if (e != hipSuccess) { (void)hipGetLastError(); return e; }   // (the caller reports it; the sticky runtime error must not fail the next launch check)
        blocks.push_back(Block{q, pinned});
        *out = q;
        return hipSuccess;
    }
public:
    DevHeap() = default;
    DevHeap(const DevHeap&) = delete;
    DevHeap& operator=(const DevHeap&) = delete;
    ~DevHeap() { release_all(); }
    // p = a fresh block of `bytes` (a block p still holds goes back first: re-reservation); p stays null when the device refuses
    template <class T> hipError_t alloc(T*& p, size_t bytes, bool pinned = false) {
        give_back(p);
        return take((void**)&p, bytes, pinned);
    }
    template <class T> hipError_t alloc_zeroed(T*& p, size_t bytes) {
        const hipError_t e = alloc(p, bytes);
        return e != hipSuccess ? e : hipMemset(p, 0, bytes);
    }
    // one block back early; the caller's pointer is nulled (a pointer this heap did not hand out is left to its owner)
    template <class T> void give_back(T*& p) {
        for (size_t i = blocks.size(); p && i-- > 0;)
            if (blocks[i].p == (void*)p) {
                if (blocks[i].pinned) hipHostFree(blocks[i].p); else hipFree(blocks[i].p);
                blocks.erase(blocks.begin() + (long)i);
                break;
            }
        p = nullptr;
    }
    // single-purpose events (the lanes own theirs)
    hipError_t event(hipEvent_t& e) {
        if (e) return hipSuccess;
        const hipError_t rc = hipEventCreate(&e);
        if (rc != hipSuccess) { e = nullptr; return rc; }
        events.push_back(e);
        return hipSuccess;
    }
    void drop_event(hipEvent_t& e) {
        const auto it = std::find(events.begin(), events.end(), e);
        if (e && it != events.end()) { hipEventDestroy(e); events.erase(it); }
        e = nullptr;
    }
    void release_all() {
        for (const Block& b : blocks) { if (b.pinned) hipHostFree(b.p); else hipFree(b.p); }
        for (hipEvent_t e : events) hipEventDestroy(e);
        blocks.clear();
        events.clear();
    }
};

// A device buffer that grows on demand (grow); cap in elements.  The block belongs to the heap it was grown from.
template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;
    operator T*() const { return p; }
};
// Room for `need` elements: 25 % headroom, never fewer than 1024; a live buffer is released only once `drain` has finished with it.
// -1 with the message in `error` when the device refuses (the buffer is then empty).
template <class T>
int grow(DevHeap& heap, DevBuf<T>& b, size_t need, hipStream_t drain, const char* what, std::string& error) {
    if (need <= b.cap) return 0;
    const size_t n = std::max(need + need / 4, (size_t)1024);
    if (b.p) hipStreamSynchronize(drain);
    b.cap = 0;
    if (heap.alloc(b.p, n * sizeof(T)) != hipSuccess) { error = std::string("out of device memory (") + what + ")"; return -1; }
    b.cap = n;
    return 0;
}

// A side stream, the ring of events that order it behind its producers, and the event its consumer waits for.  N events: more than
// one pass records, so no event is re-recorded while a wait on it can be pending.
template <int N>
struct Lane {
    hipStream_t s = nullptr;
    hipEvent_t ring[N] = {};
    hipEvent_t done = nullptr;
    int next = 0;
    Lane() = default;
    Lane(const Lane&) = delete;
    Lane& operator=(const Lane&) = delete;
    ~Lane() { destroy(); }
    operator hipStream_t() const { return s; }   // a lane stands where its stream stood (null: not created)
    // non-blocking (a blocking stream would serialise with the legacy default stream on every launch); a lane that could not be
    // completed is taken down again
    hipError_t create() {
        if (s) return hipSuccess;
        hipError_t e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
        if (e != hipSuccess) { s = nullptr; return e; }
        for (int i = 0; i < N && e == hipSuccess; ++i) e = hipEventCreate(&ring[i]);
        if (e == hipSuccess) e = hipEventCreate(&done);
        if (e != hipSuccess) destroy();
        return e;
    }
    // everything enqueued on `producer` so far happens before what is enqueued on the lane next
    void after(hipStream_t producer) {
        hipEvent_t ev = ring[next];
        next = (next + 1) % N;
        hipEventRecord(ev, producer);
        hipStreamWaitEvent(s, ev, 0);
    }
    // `consumer` waits for everything enqueued on the lane so far
    void join(hipStream_t consumer) {
        hipEventRecord(done, s);
        hipStreamWaitEvent(consumer, done, 0);
    }
    void destroy() {
        if (s) { hipStreamSynchronize(s); hipStreamDestroy(s); s = nullptr; }
        for (hipEvent_t& e : ring) if (e) { hipEventDestroy(e); e = nullptr; }
        if (done) { hipEventDestroy(done); done = nullptr; }
        next = 0;
    }
};

}  // namespace mtts
