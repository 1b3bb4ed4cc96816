// lnb_own.h -- who releases a runtime resource: the scope that holds it.  Plain C++ over standard headers only; the acquire and release
// functions are template arguments, so that tests/native/own_test.cpp can walk every type with counting ones under the sanitizers.
// lnb_api.cpp instantiates them with the runtime's own free / destroy functions.
//
//   Owned<T, Release>            one handle (a typed device pointer, a pinned host pointer, an event, a stream, a graph-exec): move-only, converts
//                                to the raw handle, released exactly once -- by reset(), by being assigned over, or when it leaves scope
//   Grown<T, Release>            a buffer that is replaced by a larger one on demand: pointer + capacity in bytes
//   Arena<E, Acquire, Release>   the buffers of one scope (an entry point's temporaries, a model's weights): released in reverse order
//   GraphTable<G, Release, L, F> the captured graphs of a context or a batch, by token launch and attention form
//
// An error code of the runtime is any type whose value-initialised value means success.
#pragma once
#include <cstddef>
#include <utility>
#include <vector>

template <class T, auto Release> class Owned {
    T h_ = T();
public:
    Owned() = default;
    explicit Owned(T h) : h_(h) {}
    Owned(const Owned&) = delete;
    Owned& operator=(const Owned&) = delete;
    Owned(Owned&& o) noexcept : h_(o.release()) {}
    Owned& operator=(Owned&& o) noexcept { if (this != &o) { reset(); h_ = o.release(); } return *this; }
    ~Owned() { reset(); }
    operator T() const { return h_; }
    T get() const { return h_; }
    void reset() { if (h_) { Release(h_); h_ = T(); } }
    T release() { T h = h_; h_ = T(); return h; }      // the caller takes the handle over
    // what it held goes first; acquire(T*) reports the runtime's code, and only a success is kept
    template <class Acquire> auto fill(Acquire acquire) -> decltype(acquire((T*)nullptr)) {
        reset();
        T h = T();
        const auto e = acquire(&h);
        if (e == decltype(e)()) h_ = h;
        return e;
    }
};

// A request that fits does nothing.  One that does not releases the old buffer, then acquires the new one (never both at once: the peak stays
// what the larger one takes); the caller has synchronised whatever still reads the old one.  A failed acquire leaves it empty with capacity 0.
template <class T, auto Release> class Grown {
    Owned<T, Release> p_;
    size_t cap_ = 0;
public:
    operator T() const { return p_.get(); }
    T get() const { return p_.get(); }
    size_t capacity() const { return cap_; }
    bool fits(size_t bytes) const { return bytes <= cap_; }
    void reset() { p_.reset(); cap_ = 0; }
    template <class Acquire> auto reserve(size_t bytes, Acquire acquire) -> decltype(acquire((T*)nullptr, bytes)) {
        if (fits(bytes)) return decltype(acquire((T*)nullptr, bytes))();
        reset();
        const auto e = p_.fill([&](T* q) { return acquire(q, bytes); });
        if (e == decltype(e)()) cap_ = bytes;
        return e;
    }
};

// alloc<T>(count) hands out a raw pointer and remembers it.  The first failure is latched: error() keeps it, every later alloc returns null
// without acquiring.  Leaving scope (or reset(), which also clears the latch) releases everything, last acquired first.
template <class E, E (*Acquire)(void**, size_t), auto Release> class Arena {
    std::vector<void*> held_;
    E err_ = E();
public:
    Arena() = default;
    Arena(const Arena&) = delete;
    Arena& operator=(const Arena&) = delete;
    ~Arena() { reset(); }
    template <class T> T* alloc(size_t count) {
        if (err_ != E()) return nullptr;
        void* p = nullptr;
        const E e = Acquire(&p, count * sizeof(T));
        if (e != E()) { err_ = e; return nullptr; }
        held_.push_back(p);
        return (T*)p;
    }
    E error() const { return err_; }
    size_t size() const { return held_.size(); }
    void reset() {
        while (!held_.empty()) { Release(held_.back()); held_.pop_back(); }
        err_ = E();
    }
};

// One slot per (token launch, attention form).  drop(form): whatever bakes that form in goes, for every launch.
template <class G, auto Release, int Launches, int Forms> class GraphTable {
    Owned<G, Release> g_[Launches][Forms];
public:
    Owned<G, Release>& slot(int launch, int form) { return g_[launch][form]; }
    void drop(int form) { for (int l = 0; l < Launches; l++) g_[l][form].reset(); }
    void drop_all() { for (int f = 0; f < Forms; f++) drop(f); }
};
