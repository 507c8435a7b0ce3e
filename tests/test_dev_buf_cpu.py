"""dev_buf.h, the owning device buffer, against malloc-backed stand-ins.

The header names the HIP runtime through six names only and includes no
runtime header, so a stand-alone host program can define those names itself
and include it. The stand-ins keep the set of live allocations, abort on a
free of a pointer they do not know, and can be told to fail the n-th
allocation or copy; the program checks dev_buf's ownership rules with them.
"""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "futuresdr_amd", "csrc")

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <utility>

enum hipError_t { hipSuccess = 0, hipErrorOutOfMemory = 2, hipErrorUnknown = 999 };
enum hipMemcpyKind { hipMemcpyHostToDevice = 1 };

static std::set<void*> live;
static int n_alloc = 0, n_copy = 0, n_free = 0;
static int fail_alloc = 0, fail_copy = 0; /* 1-based call to fail; 0 = none */

static hipError_t hipMalloc(void** p, size_t bytes) {
    if (++n_alloc == fail_alloc) { *p = (void*)0x1; return hipErrorOutOfMemory; }
    *p = malloc(bytes ? bytes : 1);
    live.insert(*p);
    return hipSuccess;
}
static hipError_t hipFree(void* p) {
    if (!live.erase(p)) {
        fprintf(stderr, "free of unknown pointer %p\n", p);
        abort();
    }
    n_free++;
    free(p);
    return hipSuccess;
}
static hipError_t hipMemcpy(void* d, const void* s, size_t n, hipMemcpyKind) {
    if (++n_copy == fail_copy) return hipErrorUnknown;
    memcpy(d, s, n);
    return hipSuccess;
}
static hipError_t hipMemset(void* d, int v, size_t n) {
    memset(d, v, n);
    return hipSuccess;
}

#include "dev_buf.h"

#define CHECK(cond)                                                    \
    do {                                                               \
        if (!(cond)) {                                                 \
            fprintf(stderr, "line %d: %s\n", __LINE__, #cond);         \
            exit(1);                                                   \
        }                                                              \
    } while (0)

int main() {
    { /* ensure keeps the buffer when the request fits, replaces it when not */
        dev_buf b;
        CHECK(b.ptr == nullptr && b.bytes == 0 && !b);
        CHECK(b.ensure(100) == hipSuccess && b.bytes == 100 && live.size() == 1);
        void* p = b.ptr;
        CHECK(b.ensure(40) == hipSuccess && b.ptr == p && b.bytes == 100);
        CHECK(b.ensure(100) == hipSuccess && b.ptr == p);
        const int frees = n_free;
        CHECK(b.ensure(101) == hipSuccess && b.bytes == 101);
        CHECK(n_free == frees + 1 && live.size() == 1 && live.count(b.ptr));
        CHECK(b.zero() == hipSuccess && b.as<char>()[100] == 0);
    }
    CHECK(live.empty());
    { /* a failed allocation leaves {nullptr, 0}; a later ensure works */
        dev_buf b;
        CHECK(b.ensure(16) == hipSuccess);
        fail_alloc = n_alloc + 1;
        CHECK(b.ensure(32) == hipErrorOutOfMemory);
        CHECK(b.ptr == nullptr && b.bytes == 0 && live.empty());
        CHECK(b.ensure(8) == hipSuccess && b.bytes == 8 && live.size() == 1);
    }
    CHECK(live.empty());
    { /* upload: exact size, contents; a failed copy leaves nothing live */
        const float h[3] = {1.f, 2.f, 3.f};
        dev_buf b;
        CHECK(b.upload(h, 3) == hipSuccess && b.bytes == sizeof(h));
        CHECK(b.as<float>()[2] == 3.f && live.size() == 1);
        fail_copy = n_copy + 1;
        CHECK(b.upload(h, 2) == hipErrorUnknown);
        CHECK(b.ptr == nullptr && b.bytes == 0 && live.empty());
        fail_alloc = n_alloc + 1;
        CHECK(b.upload(h, 3) == hipErrorOutOfMemory);
        CHECK(b.ptr == nullptr && b.bytes == 0 && live.empty());
    }
    CHECK(live.empty());
    { /* moves transfer ownership; the overwritten buffer is freed once */
        dev_buf a, c;
        CHECK(a.ensure(10) == hipSuccess && c.ensure(20) == hipSuccess);
        void *pa = a.ptr, *pc = c.ptr;
        dev_buf m(std::move(a));
        CHECK(m.ptr == pa && m.bytes == 10 && a.ptr == nullptr && a.bytes == 0);
        CHECK(live.size() == 2);
        const int frees = n_free;
        c = std::move(m);
        CHECK(n_free == frees + 1 && !live.count(pc));
        CHECK(c.ptr == pa && c.bytes == 10 && m.ptr == nullptr && m.bytes == 0);
        CHECK(live.size() == 1);
        dev_buf& self = c;
        c = std::move(self);
        CHECK(c.ptr == pa && live.size() == 1);
    }
    CHECK(live.empty()); /* and nothing is live at exit */
    puts("dev_buf ok");
    return 0;
}
"""


def test_dev_buf_ownership(tmp_path):
    cxx = (shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++")
           or shutil.which("clang++"))
    if not cxx:
        pytest.skip("no host C++ compiler")
    src = tmp_path / "dev_buf_check.cpp"
    exe = tmp_path / "dev_buf_check"
    src.write_text(PROGRAM)
    subprocess.run([cxx, "-O1", "-std=c++17", "-I", CSRC, str(src), "-o",
                    str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    assert "dev_buf ok" in run.stdout
