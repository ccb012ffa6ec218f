// Self-test of the owning buffer type (csrc/aqc_devbuf.h) over a counting policy backed by malloc, for ASan + UBSan
// (tests/test_native_sanitizers.py): every path leaves no live block, a failed allocation leaves an empty buffer, and a struct of
// buffers whose third allocation fails is released by its destructor (the early exits of aqc_ws_create).
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <utility>

#include "../../aqc_research_amd/csrc/aqc_devbuf.h"

static int g_fail_msgs = 0;
int aqc::fail(const char* fmt, ...) {
    (void)fmt;
    ++g_fail_msgs;
    return 1;
}

namespace {

long long g_live = 0, g_allocs = 0, g_frees = 0;
long long g_fail_at = 0;   // the k-th allocation from now fails (1: the next one; 0: none)

struct Counting {
    static int allocate(void** p, size_t bytes) {
        if (g_fail_at > 0 && --g_fail_at == 0) { *p = nullptr; return aqc::fail("allocation of %zu bytes refused", bytes); }
        *p = malloc(bytes ? bytes : 1);
        if (!*p) return aqc::fail("malloc failed");
        ++g_live; ++g_allocs;
        return 0;
    }
    static int deallocate(void* p) { free(p); --g_live; ++g_frees; return 0; }
    static int copy_in(void* dst, const void* host, size_t bytes) { memcpy(dst, host, bytes); return 0; }
};
template <class T> using TBuf = aqc::Buf<T, Counting>;

static_assert(!std::is_copy_constructible<TBuf<int>>::value, "a buffer has one owner");
static_assert(!std::is_copy_assignable<TBuf<int>>::value, "a buffer has one owner");
static_assert(std::is_nothrow_move_constructible<TBuf<int>>::value && std::is_nothrow_move_assignable<TBuf<int>>::value, "move-only");

int failures = 0;
#define CHECK(cond) do { if (!(cond)) { ++failures; printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); } } while (0)

struct Handle {   // a handle whose members are allocated one after the other, as a workspace's are
    TBuf<double> a, b, c, d;
    int create() { return a.alloc(8) || b.alloc(8) || c.alloc(8) || d.alloc(8) ? 1 : 0; }
};

void run() {
    {   // alloc, capacity, conversion, release
        TBuf<double> b;
        CHECK(!b && b.capacity() == 0 && static_cast<double*>(b) == nullptr);
        CHECK(b.alloc(5) == 0 && b && b.capacity() == 5 && g_live == 1);
        double* raw = b;
        raw[4] = 1.0;
        CHECK(b.alloc(3) != 0 && b.capacity() == 5 && g_live == 1);   // alloc wants an empty buffer
        CHECK(b.release() == 0 && !b && b.capacity() == 0 && g_live == 0);
        CHECK(b.release() == 0);
    }
    CHECK(g_live == 0);
    {   // reserve: grow-only
        TBuf<int> b;
        CHECK(b.reserve(0) == 0 && !b && g_allocs == 1);
        CHECK(b.reserve(4) == 0 && b.capacity() == 4);
        const long long a0 = g_allocs, f0 = g_frees;
        int* before = b;
        CHECK(b.reserve(4) == 0 && b.reserve(2) == 0 && b.reserve(0) == 0);
        CHECK(g_allocs == a0 && g_frees == f0 && static_cast<int*>(b) == before && b.capacity() == 4);   // no-op at or below capacity
        CHECK(b.reserve(9) == 0 && b.capacity() == 9);
        CHECK(g_allocs == a0 + 1 && g_frees == f0 + 1 && g_live == 1);   // one free and one allocation above it
        static_cast<int*>(b)[8] = 7;
        g_fail_at = 1;   // a failed allocation inside reserve: empty, capacity 0, non-zero
        CHECK(b.reserve(20) != 0 && !b && b.capacity() == 0 && g_live == 0);
        CHECK(b.reserve(3) == 0 && b.capacity() == 3 && g_live == 1);   // and the buffer is usable again
    }
    CHECK(g_live == 0);
    {   // upload
        TBuf<int> e, f, g;
        CHECK(e.upload({}) == 0 && e.capacity() == 1 && g_live == 1);      // an empty vector: min_count elements
        CHECK(f.upload({}, 3) == 0 && f.capacity() == 3);
        const std::vector<int> v = {1, 2, 3, 4, 5};
        CHECK(g.upload(v) == 0 && g.capacity() == 5 && static_cast<int*>(g)[0] == 1 && static_cast<int*>(g)[4] == 5);
        CHECK(g.upload(v) != 0 && g.capacity() == 5);   // upload allocates: the buffer must be empty
        g_fail_at = 1;
        TBuf<int> h;
        CHECK(h.upload(v) != 0 && !h && h.capacity() == 0);
    }
    CHECK(g_live == 0);
    {   // moves
        TBuf<double> a;
        CHECK(a.alloc(4) == 0);
        double* pa = a;
        TBuf<double> b(std::move(a));   // move construction
        CHECK(!a && a.capacity() == 0 && static_cast<double*>(b) == pa && b.capacity() == 4 && g_live == 1);
        TBuf<double> c;
        CHECK(c.alloc(6) == 0 && g_live == 2);
        c = std::move(b);               // move assignment onto a non-empty buffer: its block goes
        CHECK(g_live == 1 && static_cast<double*>(c) == pa && c.capacity() == 4 && !b && b.capacity() == 0);
        TBuf<double>& self = c;
        c = std::move(self);            // onto itself: nothing happens
        CHECK(g_live == 1 && static_cast<double*>(c) == pa);
        a = std::move(c);               // into an empty one
        CHECK(g_live == 1 && a.capacity() == 4 && !c);
    }
    CHECK(g_live == 0);   // destruction
    {   // a struct of several buffers whose third allocation fails is released by its destructor
        Handle h;
        g_fail_at = 3;
        CHECK(h.create() != 0);
        CHECK(h.a && h.b && !h.c && !h.d && g_live == 2);
    }
    CHECK(g_live == 0);
    {   // ... and a complete one by its deletion
        Handle* h = new Handle();
        CHECK(h->create() == 0 && g_live == 4);
        delete h;
    }
    CHECK(g_live == 0 && g_allocs == g_frees && g_fail_at == 0);
    CHECK(g_fail_msgs == 5);   // every refusal above went through fail(): 2 non-empty allocs, 3 refused allocations
}

}  // namespace

int main() {
    run();
    printf("devbuf selftest: %lld allocations, %lld frees, %lld live, %d failures\n", g_allocs, g_frees, g_live, failures);
    return failures == 0 ? 0 : 1;
}
