// own_test.cpp -- csrc/lnb_own.h on the host (tests/test_own_cpu.py builds it with -fsanitize=address,undefined and runs it as a child
// process).  Every type is instantiated with counting acquire and release functions: handles are the numbers 1, 2, 3, ... in the order they
// were acquired (as pointers that are never dereferenced), every release is logged, and the acquire can be told to fail on its i-th call.
#include <cstdint>
#include <cstdio>
#include <vector>
#include "../../llama-nuts-and-bolts_amd/csrc/lnb_own.h"

static int g_bad = 0;
#define CHECK(c, ...) do { if (!(c)) { if (g_bad++ < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } } while (0)

typedef int Err;                                             // 0: success
static int g_acquired = 0, g_fail_at = 0;                    // g_fail_at: the call (1-based) that fails with code 100 + i; 0: none
static std::vector<uintptr_t> g_released;                    // handles, in the order they were released
static size_t g_last_bytes = 0;
static void start(int fail_at = 0) { g_acquired = 0; g_fail_at = fail_at; g_released.clear(); g_last_bytes = 0; }
static Err acquire(void** p, size_t bytes) {
    g_acquired++; g_last_bytes = bytes;
    if (g_acquired == g_fail_at) return 100 + g_acquired;
    *p = (void*)(uintptr_t)g_acquired;
    return 0;
}
static Err release(void* p) { g_released.push_back((uintptr_t)p); return 0; }
static int times_released(uintptr_t h) { int n = 0; for (uintptr_t r : g_released) n += r == h; return n; }

typedef Owned<int*, release> Ptr;
static Err fill(Ptr& p, size_t bytes = 4) { return p.fill([&](int** q) { return acquire((void**)q, bytes); }); }

static void check_owned() {
    start();
    { Ptr p; CHECK(fill(p) == 0 && p.get() == (int*)1, "fill keeps the handle"); int* raw = p; CHECK(raw == (int*)1, "the conversion yields the handle"); }
    CHECK(g_released.size() == 1 && g_released[0] == 1, "released once on scope exit (%zu)", g_released.size());
    start();
    { Ptr p; fill(p); p.reset(); CHECK(g_released.size() == 1 && !p.get() && !p, "reset releases and empties"); p.reset(); }
    CHECK(g_released.size() == 1, "reset, reset again, scope exit: one release (%zu)", g_released.size());
    start();
    { Ptr a, b; fill(a); fill(b); a = std::move(b);
      CHECK(g_released.size() == 1 && g_released[0] == 1, "move-assignment over a full owner releases what it held");
      CHECK(a.get() == (int*)2 && !b.get(), "... and takes the other's handle, which is left empty"); }
    CHECK(g_released.size() == 2 && times_released(2) == 1, "the moved-from owner releases nothing when it goes (%zu releases)", g_released.size());
    start();
    { Ptr a; fill(a); Ptr c(std::move(a)); CHECK(!a.get() && c.get() == (int*)1, "move construction"); }
    CHECK(g_released.size() == 1, "one handle, two owners over its life, one release (%zu)", g_released.size());
    start();
    { Ptr a; fill(a); fill(a); CHECK(g_released.size() == 1 && g_released[0] == 1 && a.get() == (int*)2, "a second fill releases the first handle"); }
    start(2);
    { Ptr a; fill(a); const Err e = fill(a); CHECK(e == 102 && !a.get(), "a failed fill reports the code and leaves the owner empty (%d)", e); }
    CHECK(g_released.size() == 1, "nothing to release after a failed fill (%zu)", g_released.size());
    start();
    { Ptr a; fill(a); int* raw = a.release(); CHECK(raw == (int*)1 && !a.get(), "release() hands the handle over"); }
    CHECK(g_released.empty(), "... and the owner no longer releases it");
    start();
    { std::vector<Ptr> v; for (int i = 0; i < 9; i++) { v.emplace_back(); fill(v.back()); } }      // (the vector moves its elements as it grows)
    CHECK(g_released.size() == 9, "a vector of owners releases each handle once (%zu)", g_released.size());
    for (uintptr_t h = 1; h <= 9; h++) CHECK(times_released(h) == 1, "handle %zu released %d times", (size_t)h, times_released(h));
}

typedef Grown<char*, release> Buf;
static Err reserve(Buf& b, size_t bytes) { return b.reserve(bytes, [](char** q, size_t n) { return acquire((void**)q, n); }); }

static void check_grown() {
    start();
    {
        Buf b;
        CHECK(!b.get() && b.capacity() == 0 && b.fits(0) && !b.fits(1), "empty at first");
        CHECK(reserve(b, 0) == 0 && g_acquired == 0, "a request for nothing acquires nothing");
        CHECK(reserve(b, 100) == 0 && g_acquired == 1 && g_last_bytes == 100 && b.capacity() == 100 && b.get() == (char*)1, "first growth");
        CHECK(reserve(b, 100) == 0 && reserve(b, 7) == 0 && g_acquired == 1 && g_released.empty(), "no call when the request fits");
        CHECK(reserve(b, 101) == 0 && g_acquired == 2 && g_released.size() == 1 && g_released[0] == 1 && b.get() == (char*)2 && b.capacity() == 101,
              "release, then acquire, when it does not");
        g_fail_at = 3;
        const Err e = reserve(b, 500);
        CHECK(e == 103 && !b.get() && b.capacity() == 0 && !b.fits(1), "empty with capacity 0 after a failed growth (%d)", e);
        CHECK(g_released.size() == 2 && g_released[1] == 2, "the old buffer went before the failed acquire");
        CHECK(reserve(b, 50) == 0 && g_acquired == 4 && b.get() == (char*)4 && b.capacity() == 50, "a following smaller request acquires again");
        char* raw = b; CHECK(raw == (char*)4, "the conversion yields the pointer");
    }
    CHECK(g_released.size() == 3 && g_released[2] == 4, "the last buffer goes with the scope (%zu)", g_released.size());
    start();
    { Buf b; reserve(b, 8); b.reset(); CHECK(g_released.size() == 1 && !b.get() && b.capacity() == 0, "reset"); }
    CHECK(g_released.size() == 1, "one release after reset and scope exit");
}

typedef Arena<Err, acquire, release> Scope;

static void check_arena() {
    start();
    {
        Scope a;
        for (int i = 1; i <= 8; i++) { double* p = a.alloc<double>((size_t)i); CHECK(p == (double*)(uintptr_t)i && g_last_bytes == (size_t)i * 8, "allocation %d", i); }
        CHECK(a.error() == 0 && a.size() == 8 && g_released.empty(), "eight held, none released inside the scope");
    }
    CHECK(g_released.size() == 8, "all released at scope exit (%zu)", g_released.size());
    for (int i = 0; i < 8 && i < (int)g_released.size(); i++) CHECK(g_released[i] == (uintptr_t)(8 - i), "reverse order: release %d was of handle %zu", i, (size_t)g_released[i]);
    for (int fail = 1; fail <= 8; fail++) {
        start(fail);
        {
            Scope a;
            for (int i = 1; i <= 8; i++) {
                int* p = a.alloc<int>(3);
                CHECK((p != nullptr) == (i < fail), "failure at %d: allocation %d %s", fail, i, p ? "succeeded" : "returned null");
            }
            CHECK(g_acquired == fail, "failure at %d: later allocs acquire nothing (%d acquire calls)", fail, g_acquired);
            CHECK(a.error() == 100 + fail, "failure at %d: the latched error is the first one (%d)", fail, a.error());
            g_fail_at = 0;
            CHECK(a.alloc<int>(1) == nullptr && g_acquired == fail && a.error() == 100 + fail, "failure at %d: the latch holds when the acquire would succeed again", fail);
            CHECK(g_released.empty(), "failure at %d: nothing released before the scope ends", fail);
        }
        CHECK((int)g_released.size() == fail - 1, "failure at %d: exactly the first %d released (%zu)", fail, fail - 1, g_released.size());
        for (int i = 0; i < (int)g_released.size(); i++) CHECK(g_released[i] == (uintptr_t)(fail - 1 - i), "failure at %d: release %d was of handle %zu", fail, i, (size_t)g_released[i]);
    }
    start(2);
    { Scope a; a.alloc<int>(1); a.alloc<int>(1); a.reset();
      CHECK(g_released.size() == 1 && a.error() == 0 && a.size() == 0, "reset releases and clears the latch");
      CHECK(a.alloc<int>(1) == (int*)3, "... and the arena serves again"); }
    CHECK(g_released.size() == 2 && g_released[1] == 3, "what was acquired after a reset goes with the scope");
}

enum { LAUNCHES = 3, FORMS = 3 };
typedef GraphTable<void*, release, LAUNCHES, FORMS> Table;
static uintptr_t fill_slot(Table& t, int l, int f) { t.slot(l, f).fill([](void** q) { return acquire(q, 0); }); return (uintptr_t)t.slot(l, f).get(); }

static void check_table() {
    start();
    {
        Table t;
        for (int l = 0; l < LAUNCHES; l++) for (int f = 0; f < FORMS; f++)
            for (int l2 = 0; l2 < LAUNCHES; l2++) for (int f2 = 0; f2 < FORMS; f2++)
                CHECK((&t.slot(l, f) == &t.slot(l2, f2)) == (l == l2 && f == f2), "slots (%d, %d) and (%d, %d)", l, f, l2, f2);
        uintptr_t h[LAUNCHES][FORMS] = {};
        for (int l = 0; l < LAUNCHES; l++) for (int f = 0; f < FORMS; f++) if (!(l == 2 && f == 1)) h[l][f] = fill_slot(t, l, f);      // (2, 1) stays empty
        t.drop(1);
        CHECK(g_released.size() == 2 && times_released(h[0][1]) == 1 && times_released(h[1][1]) == 1, "drop(form) releases that form's filled slots (%zu)", g_released.size());
        for (int l = 0; l < LAUNCHES; l++) for (int f = 0; f < FORMS; f++) CHECK((t.slot(l, f).get() != nullptr) == (f != 1), "after drop(1): slot (%d, %d)", l, f);
        t.drop(1);
        CHECK(g_released.size() == 2, "dropping an empty form releases nothing");
        const uintptr_t again = fill_slot(t, 0, 1);
        CHECK(again != 0 && t.slot(0, 1).get() == (void*)again, "a slot emptied by drop can be filled again");
        t.drop_all();
        CHECK(g_released.size() == 2 + 6 + 1, "drop_all releases every filled slot (%zu)", g_released.size());
        for (int l = 0; l < LAUNCHES; l++) for (int f = 0; f < FORMS; f++) CHECK(!t.slot(l, f).get(), "after drop_all: slot (%d, %d)", l, f);
        for (uintptr_t x = 1; x <= (uintptr_t)g_acquired; x++) CHECK(times_released(x) == 1, "handle %zu released %d times", (size_t)x, times_released(x));
        fill_slot(t, 1, 2); fill_slot(t, 2, 0);
    }
    CHECK(g_released.size() == 11, "destruction releases each filled slot once (%zu)", g_released.size());
    for (uintptr_t x = 1; x <= (uintptr_t)g_acquired; x++) CHECK(times_released(x) == 1, "handle %zu released %d times", (size_t)x, times_released(x));
}

int main() {
    check_owned();
    check_grown();
    check_arena();
    check_table();
    if (g_bad) { printf("own_test: %d check(s) failed\n", g_bad); return 1; }
    printf("own_test: ok\n");
    return 0;
}
