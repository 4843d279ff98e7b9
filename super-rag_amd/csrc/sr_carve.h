// Carves one buffer into typed parts: the staging layout of a host entry point (arguments up, the
// _dev path, results down) is declared part by part, the carver adds up the bytes and, once the
// buffer exists, points every declared pointer at its part.
//
//   float *dq, *dsim;
//   int64_t* drows;
//   sr::Carve c;
//   c.part((size_t)B * dim, &dq);
//   c.part((size_t)B * k, &dsim, &drows);   // one part each, B * k elements of its own type
//   buf.carve(c);                           // DevBuf: reserve(c.bytes()), then c.bind(buf.p)
//
// Every part starts on a multiple of kAlign bytes.  A part of count 0 is legal: its pointer is valid
// to hold and compare and must not be dereferenced.  bytes() is exactly what the declared parts need
// (the end of the last one), with no slack.  Host-only and free of HIP, so a plain C++ compiler
// builds it (tests/native/carve_test.cpp).
#pragma once

#include <cstddef>
#include <stdexcept>

namespace sr {

class Carve {
 public:
  static constexpr size_t kAlign = 256;  // no coarser than the device allocator's own alignment
  static constexpr int kMaxParts = 16;

  // Declares one part of count elements for every pointer given, in the order given; *ptr points
  // at its part after bind().
  template <class... T>
  void part(size_t count, T**... ptr) {
    (one(count, ptr), ...);
  }

  size_t bytes() const { return bytes_; }

  // Points every declared pointer into the buffer at base (at least bytes() long, kAlign aligned).
  void bind(void* base) const {
    for (int i = 0; i < n_; ++i) slots_[i].set(slots_[i].ptr, static_cast<char*>(base) + slots_[i].begin);
  }

 private:
  template <class T>
  void one(size_t count, T** ptr) {
    static_assert(kAlign % alignof(T) == 0, "carve: a part's type must not need more than kAlign");
    if (n_ == kMaxParts) throw std::length_error("carve: more than kMaxParts parts");
    const size_t begin = (bytes_ + kAlign - 1) / kAlign * kAlign;
    slots_[n_++] = Slot{ptr, begin, [](void* p, char* at) {
                          *static_cast<T**>(p) = reinterpret_cast<T*>(at);
                        }};
    bytes_ = begin + count * sizeof(T);
  }
  struct Slot {
    void* ptr;  // the caller's T*
    size_t begin;
    void (*set)(void* ptr, char* at);
  };
  Slot slots_[kMaxParts];
  size_t bytes_ = 0;
  int n_ = 0;
};

}  // namespace sr
