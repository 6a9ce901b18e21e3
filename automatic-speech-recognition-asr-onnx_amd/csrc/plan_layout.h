// Layout arithmetic of a plan blob: the index tables a call uploads with one copy, as typed sections laid out in declaration order.
// Plain C++ without HIP types (PlanBlob in engine.h adds the buffers): tests/test_plan_blob_cpu.py compiles it on the CPU.
#pragma once
#include <cassert>
#include <cstddef>

struct PlanLayout {
  static constexpr int MAX_SECTIONS = 20;      // fixed capacity: building a layout allocates nothing
  size_t off[MAX_SECTIONS] = {}, bytes[MAX_SECTIONS] = {};
  int n = 0;
  size_t total = 0;
  // `count` elements of `elt` bytes behind the sections declared so far, aligned to `align` (a power of two); returns the section's index
  int add(size_t elt, size_t align, size_t count) {
    assert(n < MAX_SECTIONS && align != 0 && (align & (align - 1)) == 0);
    total = (total + align - 1) & ~(align - 1);
    off[n] = total;
    bytes[n] = elt * count;
    total += bytes[n];
    return n++;
  }
  void round_total(size_t m) { total = (total + m - 1) / m * m; }
};
