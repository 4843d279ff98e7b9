// Host test of csrc/sr_carve.h (tests/test_carve.py builds it with AddressSanitizer + UBSan and
// runs it; no GPU, no HIP).  Layouts are declared over a host buffer of exactly bytes() bytes, so a
// part that reaches past the total, a misaligned typed store or two parts that share bytes is a
// sanitizer report or a failed check.  Prints "carve_test: N layouts, 0 failures" and exits 0.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <functional>
#include <new>
#include <stdexcept>
#include <type_traits>
#include <vector>

#include "sr_carve.h"

namespace {

int g_failures = 0;
int g_layouts = 0;

#define EXPECT(cond, ...)                        \
  do {                                           \
    if (!(cond)) {                               \
      ++g_failures;                              \
      std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
      std::printf(__VA_ARGS__);                  \
      std::printf("\n");                         \
    }                                            \
  } while (0)

struct alignas(16) Vec4 {
  float x[4];
};

// One layout under test: parts are declared through add(), run() binds them to a fresh buffer of
// exactly bytes() bytes, writes every element of every part through its typed pointer, then reads
// everything back (a part overlapping another would have changed what the other wrote).
class Layout {
 public:
  explicit Layout(const char* name) : name_(name) {}

  template <class T>
  void add(T** p, size_t count) {
    c_.part(count, p);
    const int id = (int)parts_.size();
    Part part;
    part.bytes = count * sizeof(T);
    part.where = [p] { return reinterpret_cast<uintptr_t>(*p); };
    part.fill = [p, count, id] {
      for (size_t i = 0; i < count; ++i) (*p)[i] = value<T>(id, i);
    };
    part.check = [p, count, id] {
      for (size_t i = 0; i < count; ++i)
        if (!same((*p)[i], value<T>(id, i))) return false;
      return true;
    };
    parts_.push_back(part);
  }

  size_t run() {
    ++g_layouts;
    const size_t total = c_.bytes();
    char* buf = static_cast<char*>(::operator new(total, std::align_val_t(sr::Carve::kAlign)));
    c_.bind(buf);
    const uintptr_t base = reinterpret_cast<uintptr_t>(buf);
    uintptr_t end = base;  // the end of the parts so far
    for (size_t i = 0; i < parts_.size(); ++i) {
      const uintptr_t at = parts_[i].where();
      EXPECT(at % sr::Carve::kAlign == 0, "%s: part %zu starts at offset %zu", name_, i, (size_t)(at - base));
      EXPECT(at >= end, "%s: part %zu overlaps the part before it", name_, i);
      EXPECT(at - end < sr::Carve::kAlign, "%s: part %zu leaves a gap of a whole unit", name_, i);
      EXPECT(at + parts_[i].bytes <= base + total, "%s: part %zu ends past bytes()", name_, i);
      end = at + parts_[i].bytes;
    }
    EXPECT(end == base + total, "%s: bytes() = %zu, the last part ends at %zu", name_, total, (size_t)(end - base));
    for (auto& p : parts_) p.fill();
    for (size_t i = 0; i < parts_.size(); ++i)
      EXPECT(parts_[i].check(), "%s: part %zu was overwritten by another part", name_, i);
    ::operator delete(buf, std::align_val_t(sr::Carve::kAlign));
    return total;
  }

 private:
  template <class T>
  static T value(int part, size_t i) {
    if constexpr (std::is_same_v<T, Vec4>) {
      const float v = (float)(part * 1000 + (int)(i % 997));
      return Vec4{{v, v + 0.25f, v + 0.5f, v + 0.75f}};
    } else {
      return (T)(part * 1000 + (int)(i % 997));
    }
  }
  template <class T>
  static bool same(const T& a, const T& b) {
    if constexpr (std::is_same_v<T, Vec4>)
      return std::equal(a.x, a.x + 4, b.x);
    else
      return a == b;
  }
  struct Part {
    size_t bytes;
    std::function<uintptr_t()> where;
    std::function<void()> fill;
    std::function<bool()> check;
  };
  const char* name_;
  sr::Carve c_;
  std::vector<Part> parts_;
};

// ---- the layouts of the host entry points, at the shapes (B, k, dim) ----------------------------------
void store_layouts(size_t B, size_t k, size_t dim) {
  const size_t k_cand = 4 * k + 1, gs = 3, n = 2 * B + 1;
  {
    Layout l("store.get");
    int64_t* rows;
    float* out;
    l.add(&rows, n);
    l.add(&out, n * dim);
    l.run();
  }
  {
    Layout l("store.search");
    float *dq, *dsim;
    int64_t* drows;
    l.add(&dq, B * dim);
    l.add(&dsim, B * k);
    l.add(&drows, B * k);
    l.run();
  }
  {
    Layout l("store.search_subset lists");
    int64_t *off, *rows;
    int32_t* meta;
    l.add(&off, n + 1);
    l.add(&rows, 41);
    l.add(&meta, B + 17 * n + 2 * 3);
    l.run();
  }
  {
    Layout l("store.search_mmr");
    float *dq, *csim, *dscore, *dsim;
    int64_t *crows, *drows;
    l.add(&dq, B * dim);
    l.add(&crows, B * k_cand);
    l.add(&csim, B * k_cand);
    l.add(&drows, B * k);
    l.add(&dscore, B * k);
    l.add(&dsim, B * k);
    l.run();
  }
  {
    Layout l("store.group state");
    uint64_t* found;
    int32_t* ng;
    l.add(&found, B * k);
    l.add(&ng, B);
    l.run();
  }
  {
    Layout l("store.search_grouped");
    const size_t nc = B * k_cand, no = B * k * gs, nk = B * k;
    float *dq, *csim, *osim, *nsim[2];
    int64_t *crows, *orows, *nrows[2];
    uint64_t* found;
    int32_t *ogrp, *ng, *comp;
    l.add(&dq, B * dim);
    l.add(&crows, nc);
    l.add(&csim, nc);
    l.add(&orows, no);
    l.add(&osim, no);
    for (int i = 0; i < 2; ++i) {
      l.add(&nrows[i], no);
      l.add(&nsim[i], no);
    }
    l.add(&found, nk);
    l.add(&ogrp, nk);
    l.add(&ng, B);
    l.add(&comp, B);
    l.run();
  }
  {
    Layout l("store.score_rows");
    float *dq, *dsim;
    int64_t* drows;
    l.add(&dq, B * dim);
    l.add(&drows, B * k);
    l.add(&dsim, B * k);
    l.run();
  }
}

void capi_layouts(size_t B, size_t k, size_t dim) {
  const size_t ld = (dim + 63) / 64 * 64, K = 2 * k + 1;
  {
    Layout l("mmr_rerank");
    float *q32, *c32, *ds;
    uint16_t *q16, *c16;  // fp16 rows
    int32_t *dn, *di;
    l.add(&q32, B * dim);
    l.add(&c32, B * K * dim);
    l.add(&q16, B * ld);
    l.add(&c16, B * K * ld);
    l.add(&dn, B);
    l.add(&ds, B * k);
    l.add(&di, B * k);
    l.run();
  }
  {
    Layout l("rrf_fuse");
    int64_t *da, *db, *dr;
    double* ds;
    l.add(&da, B * k);
    l.add(&db, B * (k + 2));
    l.add(&ds, B * K);
    l.add(&dr, B * K);
    l.run();
  }
  {
    Layout l("hybrid_search");
    float *dq, *dsim, *lsc;
    int64_t *drow, *lrow, *orow;
    double* os;
    l.add(&dq, B * dim);
    l.add(&dsim, B * k);
    l.add(&drow, B * k);
    l.add(&lsc, B * k);
    l.add(&lrow, B * k);
    l.add(&os, B * K);
    l.add(&orow, B * K);
    l.run();
  }
  for (const size_t ka : {k, (size_t)0}) {  // an empty list a: three zero-count parts in front
    Layout l("score_fuse_sides");
    const size_t na = B * ka, nb = B * (k + 2), no = B * K;
    int64_t *da_r, *db_r, *do_r;
    float *da_s, *db_s, *dside, *dsideb, *do_s, *do_a, *do_b;
    l.add(&da_r, na);
    l.add(&da_s, na);
    l.add(&dsideb, na);
    l.add(&db_r, nb);
    l.add(&db_s, nb);
    l.add(&dside, nb);
    l.add(&do_r, no);
    l.add(&do_s, no);
    l.add(&do_a, no);
    l.add(&do_b, no);
    l.run();
  }
  {
    Layout l("hybrid_search_fused");
    const size_t ne = B * k, no = B * K;
    float *dq, *dsim, *lsc, *side, *sideb, *os, *oa, *ob;
    int64_t *drow, *lrow, *orow;
    l.add(&dq, B * dim);
    l.add(&drow, ne);
    l.add(&dsim, ne);
    l.add(&sideb, ne);
    l.add(&lrow, ne);
    l.add(&lsc, ne);
    l.add(&side, ne);
    l.add(&orow, no);
    l.add(&os, no);
    l.add(&oa, no);
    l.add(&ob, no);
    l.run();
  }
}

void lex_and_encoder_layouts(size_t B, size_t k) {
  for (const bool fixed : {false, true}) {
    Layout l("lex.search");
    float* ds;
    int64_t* dr;
    uint32_t* dfx = nullptr;
    l.add(&ds, B * k);
    l.add(&dr, B * k);
    if (fixed) l.add(&dfx, B * k);
    l.run();
    EXPECT(fixed == (dfx != nullptr), "lex.search: an undeclared part stays null");
  }
  for (const size_t nt : {(size_t)0, 2 * B + 1}) {  // no scored term at all: three zero-count parts
    Layout l("lex.score_rows tables");
    int* off;
    int32_t *t, *m;
    float* idf;
    l.add(&off, B + 1);
    l.add(&t, nt);
    l.add(&idf, nt);
    l.add(&m, nt);
    l.run();
  }
  for (const bool types : {false, true}) {
    Layout l("encoder.forward");
    const size_t S = 5;
    int32_t *ids, *mask, *tt = nullptr;
    float* out;
    l.add(&ids, B * S);
    l.add(&mask, B * S);
    if (types) l.add(&tt, B * S);
    l.add(&out, B * 3);
    l.run();
  }
}

void general_layouts() {
  {
    Layout l("single part");
    uint8_t* p;
    l.add(&p, 1);
    EXPECT(l.run() == 1, "a single one-byte part needs one byte");
  }
  {
    Layout l("single empty part");
    double* p;
    l.add(&p, 0);
    EXPECT(l.run() == 0, "an empty layout needs no bytes");
  }
  {
    Layout l("nothing declared");
    EXPECT(l.run() == 0, "no parts, no bytes");
  }
  {
    Layout l("mixed widths with empty parts between and at the end");
    uint8_t* a;
    Vec4* v;
    double* d;
    uint16_t* h;
    int64_t *e0, *e1;
    float* e2;
    l.add(&a, 1);
    l.add(&e0, 0);
    l.add(&v, 3);
    l.add(&h, 257);
    l.add(&e1, 0);
    l.add(&d, 33);
    // 1 -> 256 (+48) -> 512 (+514) -> 1280 (+264): an empty part shares the next part's start
    EXPECT(l.run() == 1280 + 33 * 8, "the total is the end of the last part");
    EXPECT((void*)e0 == (void*)v && (void*)e1 == (void*)d, "an empty part shares the next part's start");
    l.add(&e2, 0);  // an empty part at the end: one past the end of the buffer, on a boundary
    EXPECT(l.run() == 1792, "a trailing empty part ends the layout on its boundary");
  }
  {
    Layout l("exact multiples of the unit");
    float *a, *b;
    l.add(&a, 64);
    l.add(&b, 128);
    EXPECT(l.run() == 768, "parts that end on a boundary leave no padding");
  }
  {
    sr::Carve c;
    int* p[sr::Carve::kMaxParts + 1];
    bool threw = false;
    try {
      for (int i = 0; i <= sr::Carve::kMaxParts; ++i) c.part(1, &p[i]);
    } catch (const std::length_error&) {
      threw = true;
    }
    ++g_layouts;
    EXPECT(threw, "declaring more than kMaxParts parts is an error");
  }
  {
    // several pointers in one call: one part each, in the order given, as if declared one by one
    sr::Carve one, many;
    float *a1, *a2;
    int64_t *b1, *b2;
    uint8_t *c1, *c2;
    one.part(5, &a1);
    one.part(5, &b1);
    one.part(5, &c1);
    many.part(5, &a2, &b2, &c2);
    alignas(256) static char buf[1024];
    one.bind(buf);
    many.bind(buf);
    ++g_layouts;
    EXPECT(one.bytes() == many.bytes() && many.bytes() == 512 + 5, "three parts of five elements");
    EXPECT(a1 == a2 && b1 == b2 && c1 == c2, "one call with three pointers declares the same three parts");
    EXPECT((char*)b2 == buf + 256 && (char*)c2 == buf + 512, "each on its own boundary");
  }
}

}  // namespace

int main() {
  general_layouts();
  for (const auto& s : {std::vector<size_t>{1, 1, 3}, std::vector<size_t>{3, 5, 20}}) {
    store_layouts(s[0], s[1], s[2]);
    capi_layouts(s[0], s[1], s[2]);
    lex_and_encoder_layouts(s[0], s[1]);
  }
  std::printf("carve_test: %d layouts, %d failures\n", g_layouts, g_failures);
  return g_failures ? 1 : 0;
}
