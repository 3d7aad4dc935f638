"""csrc/hip_owned.h on its own, in a host program: the owning handle types the engine keeps its device memory, pinned memory,
streams and events in, instantiated with a counting fake policy in place of HIP's.  The program is built with the host
sanitizers (a handle is a malloc'ed byte, so a double free, a leak or a use after free is seen) and once without them."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "deeprecsys_amd", "csrc")

OWNED_MAIN = r"""
#include "hip_owned.h"
#include <stdio.h>
#include <stdlib.h>
#include <utility>
#include <vector>
using namespace drs;
static int fails = 0;
#define CHECK(c) do { if (!(c)) { if (++fails < 40) printf("line %d: %s\n", __LINE__, #c); } } while (0)

// the fake: a handle is a malloc'ed byte (so the sanitizer sees a double free or a leak), made and freed under a count;
// `fail_next` makes the next create fail as hipErrorOutOfMemory would, leaving *out alone
static int made = 0, freed = 0, fail_next = 0;
struct FakeMem {
  static int create(void** p, size_t bytes) {
    if (fail_next) { --fail_next; return 2; }
    *p = malloc(bytes ? bytes : 1);
    ++made;
    return 0;
  }
  static int create(void** p, size_t bytes, unsigned) { return create(p, bytes); }
  static void free(void* p) { ::free(p); ++freed; }
};
struct FakeHandle {
  static int create(char** h, unsigned) { void* p = nullptr; const int r = FakeMem::create(&p, 1); if (!r) *h = static_cast<char*>(p); return r; }
  static void free(char* h) { FakeMem::free(h); }
};
template <class T> using Buf = Buffer<T, FakeMem>;
using Handle = Owned<char*, FakeHandle>;
static int alive() { return made - freed; }

static void nulls_free_nothing() {
  const int m0 = made, f0 = freed;
  const int64_t c0 = live_objects();
  {
    Buf<float> a;                      // default-constructed
    CHECK(!a && a.get() == nullptr);
    Buf<float> b;
    CHECK(b.alloc(16) == 0 && b && live_objects() == c0 + 1);
    float* raw = b;                    // converts to the raw pointer
    raw[15] = 1.0f;
    CHECK(b[15] == 1.0f && b + 1 == raw + 1);
    Buf<float> c(std::move(b));        // moved-from: null, frees nothing
    CHECK(!b && c.get() == raw && live_objects() == c0 + 1);
    float* out = c.release();          // released: null, frees nothing
    CHECK(!c && out == raw && live_objects() == c0 && freed == f0);
    FakeMem::free(out);                // (the caller's to free now)
  }
  CHECK(made == m0 + 1 && freed == f0 + 1 && live_objects() == c0);
}

static void move_assign_and_reset() {
  const int f0 = freed;
  const int64_t c0 = live_objects();
  {
    Buf<int> a, b;
    CHECK(a.alloc(4) == 0 && b.alloc(4) == 0 && live_objects() == c0 + 2);
    int* pb = b;
    a = std::move(b);                  // the target's old handle is freed exactly once
    CHECK(freed == f0 + 1 && a.get() == pb && !b && live_objects() == c0 + 1);
    Buf<int>& self = a;
    a = std::move(self);               // self-move: harmless
    CHECK(freed == f0 + 1 && a.get() == pb && live_objects() == c0 + 1);
    void* fresh = nullptr;
    CHECK(FakeMem::create(&fresh, 16) == 0);
    a.reset(static_cast<int*>(fresh)); // reset(new) frees the old handle and takes the new one over
    CHECK(freed == f0 + 2 && a.get() == fresh && live_objects() == c0 + 1);
    a.reset();
    CHECK(freed == f0 + 3 && !a && live_objects() == c0);
    a.reset();                         // ... and a null object frees nothing
    CHECK(freed == f0 + 3);
  }
  CHECK(freed == f0 + 3 && alive() == 0 && live_objects() == c0);
}

static void failed_alloc() {
  const int m0 = made, f0 = freed;
  const int64_t c0 = live_objects();
  Buf<double> a;
  fail_next = 1;
  CHECK(a.alloc(8) == 2 && !a && live_objects() == c0 && made == m0 && freed == f0);
  Handle h;
  fail_next = 1;
  CHECK(h.create(0u) == 2 && !h && live_objects() == c0);
  CHECK(h.create(0u) == 0 && h && live_objects() == c0 + 1);
  Buf<void> bytes;                     // void: the count is bytes
  CHECK(bytes.alloc(3, 1u) == 0 && bytes && live_objects() == c0 + 2);
  fail_next = 1;
  CHECK(bytes.alloc(3) == 2 && !bytes && live_objects() == c0 + 1);   // what was held is freed before the new one is made
  h.reset();
  CHECK(alive() == 0 && live_objects() == c0);
}

// a struct of such members in a vector, as the engine's slots are
struct Slot {
  Handle stream;
  Buf<float> T, R;
  Handle ev[3];
  int tag = 0;
};
static int build(Slot& s, int tag) {
  int r;
  if ((r = s.stream.create(1u)) || (r = s.T.alloc(32)) || (r = s.R.alloc(8))) return r;
  for (auto& ev : s.ev) if ((r = ev.create(0u))) return r;
  s.tag = tag;
  return 0;
}
static void vector_of_slots() {
  const int m0 = made, f0 = freed;
  const int64_t c0 = live_objects();
  {
    std::vector<Slot> v;
    v.resize(3);
    for (int i = 0; i < 3; ++i) CHECK(build(v[(size_t)i], i) == 0);
    CHECK(live_objects() == c0 + 18);
    float* t1 = v[1].T;
    v.resize(40);                      // up: the elements move to new storage, nothing is freed
    CHECK(freed == f0 && v[1].T.get() == t1 && v[1].tag == 1 && !v[39].T && live_objects() == c0 + 18);
    CHECK(build(v[39], 39) == 0 && live_objects() == c0 + 24);
    v.resize(2);                       // down: slots 2 and 39 go, each handle once
    CHECK(freed == f0 + 12 && live_objects() == c0 + 12);
    v.shrink_to_fit();
    CHECK(freed == f0 + 12 && v[1].T.get() == t1);
  }
  CHECK(made == m0 + 24 && freed == f0 + 24 && live_objects() == c0);
}

// a function that returns between two allocations, as a failing HIP_TRY does
#define TRY(call) do { const int _r = (call); if (_r) return _r; } while (0)
static int two_step(int fail_at) {
  Buf<float> first, second;
  Handle ev;
  fail_next = fail_at == 0;
  TRY(first.alloc(64));
  fail_next = fail_at == 1;
  TRY(second.alloc(64));
  fail_next = fail_at == 2;
  TRY(ev.create(0u));
  return 0;
}
static void early_returns() {
  const int64_t c0 = live_objects();
  for (int at = 0; at < 4; ++at) {
    CHECK(two_step(at) == (at < 3 ? 2 : 0));
    CHECK(alive() == 0 && live_objects() == c0);
  }
}

int main() {
  nulls_free_nothing();
  move_assign_and_reset();
  failed_alloc();
  vector_of_slots();
  early_returns();
  CHECK(alive() == 0 && live_objects() == 0);
  printf("%d failures (%d handles made)\n", fails, made);
  return fails != 0;
}
"""


@pytest.fixture(scope="module")
def owned_main(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a C++ compiler builds the host program"
    d = tmp_path_factory.mktemp("hip_owned")
    src = d / "owned_main.cpp"
    src.write_text(OWNED_MAIN)

    def build(name, *flags):
        exe = d / name
        r = subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-g", "-I", CSRC] + list(flags) + [str(src), "-o", str(exe)],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        return str(exe)
    return build


def test_the_owning_handles_under_the_host_sanitizers(owned_main):
    """the header alone with -fsanitize=address,undefined, run directly, over a counting fake policy: null, moved-from and
    released objects free nothing; move-assign and reset free the old handle once; a failed alloc leaves a null object;
    a vector of structs of handles survives resize; an early return between two allocations leaves nothing behind"""
    exe = owned_main("owned_main_san", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                     "-static-libasan", "-static-libubsan")
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "0 failures" in r.stdout, r.stdout + r.stderr


def test_the_same_program_without_the_sanitizers(owned_main):
    exe = owned_main("owned_main_o3", "-O3")
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "0 failures" in r.stdout, r.stdout + r.stderr


def test_the_engine_frees_nothing_by_hand():
    """no hipFree / hipHostFree / hipEventDestroy / hipStreamDestroy call in the engine's host files outside hip_owned.h
    (the owning types) and engine_arena.hip (the table arenas, handle structs by design); the header's generic part is
    plain C++"""
    names = sorted(n for n in os.listdir(CSRC) if re.match(r"engine.*\.(hip|h)$|device_rows\.hip$", n))
    assert "engine_create.hip" in names and "engine_rows.hip" in names and "device_rows.hip" in names
    found = []
    for name in names:
        if name == "engine_arena.hip":
            continue
        for no, line in enumerate(open(os.path.join(CSRC, name)).read().split("\n"), 1):
            if re.search(r"\bhip(Free|HostFree|EventDestroy|StreamDestroy)\s*\(", re.sub(r"//.*", "", line)):
                found.append((name, no, line.strip()))
    assert found == [], found
    hdr = open(os.path.join(CSRC, "hip_owned.h")).read()
    generic = re.sub(r"//.*", "", hdr.split("#if defined(__HIPCC__)")[0])
    assert "hip" not in generic.lower()
    assert "hip_owned.h" in open(os.path.join(CSRC, "Makefile")).read()
