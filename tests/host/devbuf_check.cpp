// devbuf_check.cpp — csrc/qoc_devbuf.hpp on its own: allocate, grow, release, move-in and scope exit, with a request
// that cannot be had (SIZE_MAX / 2 bytes) among them.  After every call, whichever way it went (on a machine without a
// device every allocation fails), the invariants are checked:
//   - a buffer's pointer is null exactly when its size is 0;
//   - the ledger equals the sum of the live counted buffers;
//   - a failed alloc / grow leaves the buffer empty, not dangling;
//   - a second release changes nothing.
// Exit status 1 on a violation (each is printed), 0 otherwise.  tests/test_devbuf_host.py compiles and runs it.
#include <cstdint>
#include <cstdio>
#include <utility>
#include <vector>

#include "../../quantumoptimalcontrol.jl_amd/csrc/qoc_devbuf.hpp"

using namespace qoc;

static int violations = 0;
static int allocated = 0;  // calls that got memory (0 on a machine without a device)

#define EXPECT(cond, what)                                             \
  do {                                                                 \
    if (!(cond)) {                                                     \
      std::printf("line %d: %s: %s\n", __LINE__, what, #cond);         \
      ++violations;                                                    \
    }                                                                  \
  } while (0)

struct Probe {
  const DevBuf<char>* b;
  bool counted;
};

static void invariants(const char* what, const DevLedger& L, const std::vector<Probe>& bufs) {
  size_t sum = 0;
  for (const Probe& p : bufs) {
    EXPECT(((char*)*p.b == nullptr) == (p.b->bytes() == 0), what);
    if (p.counted) sum += p.b->bytes();
  }
  EXPECT(L.bytes == sum, what);
}

// one alloc / grow: success means exactly / at least n bytes, failure means empty
static bool sized(const char* what, DevBuf<char>& b, hipError_t e, size_t n, bool exact) {
  if (e == hipSuccess) {
    EXPECT((char*)b != nullptr && (exact ? b.bytes() == n : b.bytes() >= n), what);
    ++allocated;
    return true;
  }
  EXPECT((char*)b == nullptr && b.bytes() == 0, what);
  return false;
}

int main() {
  const size_t huge = SIZE_MAX / 2;
  DevLedger L;
  {
    DevBuf<char> a(L, kCounted), b(L, kCounted), u(L, kUncounted), h(L, kUncounted, hipHostMallocDefault);
    const std::vector<Probe> all = {{&a, true}, {&b, true}, {&u, false}, {&h, false}};
    EXPECT(L.bufs.size() == 4, "registration");
    invariants("fresh", L, all);

    sized("alloc", a, a.alloc(1024), 1024, true);
    invariants("alloc", L, all);
    {
      char* before = a;
      const size_t nb = a.bytes();
      EXPECT(a.grow(512) == hipSuccess || nb == 0, "grow within the size");
      if (nb) EXPECT((char*)a == before && a.bytes() == nb, "grow within the size keeps the buffer");
      invariants("grow within the size", L, all);
    }
    sized("grow", a, a.grow(4096), 4096, false);
    invariants("grow", L, all);
    sized("second counted buffer", b, b.alloc(300), 300, true);
    invariants("second counted buffer", L, all);

    EXPECT(a.grow(huge) != hipSuccess, "grow to SIZE_MAX / 2 must fail");
    EXPECT((char*)a == nullptr && a.bytes() == 0, "a failed grow leaves the buffer empty");
    invariants("failed grow", L, all);
    sized("alloc after a failure", a, a.alloc(64), 64, true);
    EXPECT(a.alloc(huge) != hipSuccess, "alloc of SIZE_MAX / 2 must fail");
    EXPECT((char*)a == nullptr && a.bytes() == 0, "a failed alloc leaves the buffer empty");
    invariants("failed alloc", L, all);
    EXPECT(a.alloc(0) == hipSuccess && (char*)a == nullptr, "alloc(0) is the empty buffer");
    invariants("alloc(0)", L, all);

    sized("uncounted", u, u.alloc(256), 256, true);
    invariants("uncounted", L, all);
    EXPECT(u.grow(huge) != hipSuccess && (char*)u == nullptr, "failed grow, uncounted");
    invariants("failed grow, uncounted", L, all);
    sized("pinned host", h, h.alloc(64), 64, true);
    if ((char*)h) ((char*)h)[63] = 1;  // host memory
    invariants("pinned host", L, all);
    EXPECT(h.alloc(huge) != hipSuccess && (char*)h == nullptr, "failed pinned alloc");
    invariants("failed pinned alloc", L, all);

    // release, twice
    sized("alloc before release", a, a.alloc(2048), 2048, true);
    a.release();
    EXPECT((char*)a == nullptr && a.bytes() == 0, "release");
    invariants("release", L, all);
    const size_t led = L.bytes;
    a.release();
    EXPECT(L.bytes == led && (char*)a == nullptr, "a second release is a no-op");
    invariants("second release", L, all);

    // move-in: built elsewhere, committed on success; the local is left empty and frees nothing at scope exit
    sized("alloc before move-in", a, a.alloc(1024), 1024, true);
    {
      DevBuf<char> t;  // uncounted, no ledger
      const bool got = sized("local", t, t.alloc(3000), 3000, true);
      invariants("local alive", L, all);  // (the local is nobody's)
      char* moved = t;
      a.adopt(std::move(t));
      EXPECT((char*)t == nullptr && t.bytes() == 0, "the source of a move-in is empty");
      EXPECT((char*)a == moved && a.bytes() == (got ? 3000u : 0u), "move-in takes pointer and size");
      invariants("move-in", L, all);
    }
    invariants("after the local's scope", L, all);
    {
      DevBuf<char> t;  // an early return's case: never committed
      sized("abandoned local", t, t.alloc(512), 512, true);
      EXPECT(t.alloc(huge) != hipSuccess && (char*)t == nullptr, "failed alloc, local");
      sized("abandoned local again", t, t.alloc(512), 512, true);
    }
    invariants("abandoned local", L, all);
    {
      // counted to counted: the bytes move from one ledger entry to the other
      DevBuf<char> t(L, kCounted);
      sized("counted source", t, t.alloc(700), 700, true);
      std::vector<Probe> more = all;
      more.push_back({&t, true});
      invariants("counted source", L, more);
      b.adopt(std::move(t));
      invariants("counted move-in", L, more);
      EXPECT(L.bufs.size() == 5, "registration of a scoped member");
    }
    EXPECT(L.bufs.size() == 4, "scope exit unregisters");
    invariants("scope exit of a counted buffer", L, all);
    {
      DevBuf<char> s(L, kCounted);
      sized("scoped counted", s, s.alloc(128), 128, true);
    }
    invariants("scope exit frees and uncounts", L, all);

    L.release_all();
    for (const Probe& p : all) EXPECT((char*)*p.b == nullptr && p.b->bytes() == 0, "release_all");
    EXPECT(L.bytes == 0, "release_all empties the ledger");
    sized("alloc after release_all", a, a.alloc(96), 96, true);
    invariants("alloc after release_all", L, all);
  }
  EXPECT(L.bufs.empty() && L.bytes == 0, "every buffer gone, ledger 0");
  std::printf("devbuf_check: %d violation(s), %d allocation(s) succeeded\n", violations, allocated);
  return violations ? 1 : 0;
}
