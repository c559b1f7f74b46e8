// Host-only replay harness of the native host code (csrc/host_db.cpp, host_group.cpp, host_refine.cpp, host_stage.cpp): no
// Python, no HIP.  Built by `make -C comic-text-detector_amd/csrc san OUT=<dir>` in three flavours (plain / asan / tsan) and
// driven by tests/test_host_sanitizers.py; the case files come from tests/host_replay.py.
//
//   host_replay <cases> <results> serial       every case once, one after the other
//   host_replay <cases> <results> threads N    every case TWICE (work item i = case i / 2, copy i % 2) over N threads that
//                                              draw items with a fetch-add, the loop of `parallel_for` in csrc/tail.hip: both
//                                              copies of a case are in flight at once, each with buffers of its own, and the
//                                              first call of every entry point happens under contention
//
// Every buffer an entry point sees -- inputs and outputs -- is a heap allocation of its own of EXACTLY the recorded size, so
// a sanitizer's red zone follows its last element; output pools have exactly the capacity the case states (the recorder
// states the minimum include/ctd_hip.h documents).  File format, cases and results alike (little endian):
//   file  = "CTDRPLY1" case*
//   case  = str name, str entry, u32 n_items, item*
//   item  = str tag, u8 dtype (one of "bhilILfd": u8 i16 i32 i64 u32 u64 f32 f64), u8 present (0 = a NULL pointer),
//           u32 ndim, u64 dims[ndim], bytes
//   str   = u32 length, bytes
#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <memory>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "../../include/ctd_hip.h"
#include "host_refine.h"

namespace {

struct Item {
  std::string tag;
  char dt = 'b';
  bool present = true;
  std::vector<uint64_t> dims;
  std::vector<char> bytes;
};
struct Case {
  std::string name, entry;
  std::vector<Item> items;
};

size_t dt_size(char dt) {
  switch (dt) {
    case 'b': return 1;
    case 'h': return 2;
    case 'i': case 'I': case 'f': return 4;
    case 'l': case 'L': case 'd': return 8;
  }
  throw std::runtime_error(std::string("unknown dtype ") + dt);
}

// ---- file i/o ---------------------------------------------------------------------------------------------------------
void rd(FILE* f, void* p, size_t n) {
  if (n && std::fread(p, 1, n, f) != n) throw std::runtime_error("truncated case file");
}
template <class T> T rd(FILE* f) {
  T v;
  rd(f, &v, sizeof(v));
  return v;
}
std::string rd_str(FILE* f) {
  std::string s(rd<uint32_t>(f), '\0');
  rd(f, &s[0], s.size());
  return s;
}
std::vector<Case> read_cases(const char* path) {
  FILE* f = std::fopen(path, "rb");
  if (!f) throw std::runtime_error(std::string("cannot open ") + path);
  char magic[8];
  rd(f, magic, 8);
  if (std::memcmp(magic, "CTDRPLY1", 8)) throw std::runtime_error("not a case file");
  std::vector<Case> out;
  for (int c = std::fgetc(f); c != EOF; c = std::fgetc(f)) {
    std::ungetc(c, f);
    Case cs;
    cs.name = rd_str(f);
    cs.entry = rd_str(f);
    const uint32_t n = rd<uint32_t>(f);
    for (uint32_t i = 0; i < n; ++i) {
      Item it;
      it.tag = rd_str(f);
      it.dt = (char)rd<uint8_t>(f);
      it.present = rd<uint8_t>(f) != 0;
      it.dims.resize(rd<uint32_t>(f));
      size_t count = 1;
      for (auto& d : it.dims) d = rd<uint64_t>(f), count *= (size_t)d;
      it.bytes.resize(it.present ? count * dt_size(it.dt) : 0);
      rd(f, it.bytes.data(), it.bytes.size());
      cs.items.push_back(std::move(it));
    }
    out.push_back(std::move(cs));
  }
  std::fclose(f);
  return out;
}
void wr(FILE* f, const void* p, size_t n) {
  if (n && std::fwrite(p, 1, n, f) != n) throw std::runtime_error("short write");
}
template <class T> void wr(FILE* f, T v) { wr(f, &v, sizeof(v)); }
void wr_str(FILE* f, const std::string& s) {
  wr<uint32_t>(f, (uint32_t)s.size());
  wr(f, s.data(), s.size());
}
void write_case(FILE* f, const Case& c) {
  wr_str(f, c.name);
  wr_str(f, c.entry);
  wr<uint32_t>(f, (uint32_t)c.items.size());
  for (const Item& it : c.items) {
    wr_str(f, it.tag);
    wr<uint8_t>(f, (uint8_t)it.dt);
    wr<uint8_t>(f, it.present);
    wr<uint32_t>(f, (uint32_t)it.dims.size());
    for (uint64_t d : it.dims) wr<uint64_t>(f, d);
    wr(f, it.bytes.data(), it.bytes.size());
  }
}

// ---- buffers: one exact-size heap allocation each ------------------------------------------------------------------------
struct Buf {
  std::unique_ptr<char[]> mem;   // null = a NULL pointer argument
  size_t bytes = 0;
  template <class T> T* as() const { return reinterpret_cast<T*>(mem.get()); }
};
Buf alloc(size_t bytes) {
  Buf b;
  b.mem.reset(new char[bytes]);
  b.bytes = bytes;
  if (bytes) std::memset(b.mem.get(), 0, bytes);
  return b;
}
const Item& find(const Case& c, const char* tag) {
  for (const Item& it : c.items)
    if (it.tag == tag) return it;
  throw std::runtime_error(c.name + ": no item '" + tag + "'");
}
Buf input(const Case& c, const char* tag, char dt) {
  const Item& it = find(c, tag);
  if (it.dt != dt) throw std::runtime_error(c.name + ": item '" + tag + "' has dtype " + it.dt);
  if (!it.present) return Buf();
  Buf b = alloc(it.bytes.size());
  if (!it.bytes.empty()) std::memcpy(b.mem.get(), it.bytes.data(), it.bytes.size());
  return b;
}
template <class T> T scalar(const Case& c, const char* tag, char dt) {
  const Item& it = find(c, tag);
  if (it.dt != dt || it.bytes.size() != sizeof(T)) throw std::runtime_error(c.name + ": bad scalar '" + tag + "'");
  T v;
  std::memcpy(&v, it.bytes.data(), sizeof(T));
  return v;
}
int32_t i32(const Case& c, const char* tag) { return scalar<int32_t>(c, tag, 'i'); }

void put(Case& r, const char* tag, char dt, const void* p, size_t count) {
  Item it;
  it.tag = tag, it.dt = dt, it.dims = {count};
  if (count) it.bytes.assign((const char*)p, (const char*)p + count * dt_size(dt));
  r.items.push_back(std::move(it));
}
void put_i32(Case& r, const char* tag, int32_t v) { put(r, tag, 'i', &v, 1); }

// ---- the entry points -----------------------------------------------------------------------------------------------------
void run_group_output(const Case& c, Case& r) {
  const int32_t n_blk = i32(c, "n_blk"), n_lines = i32(c, "n_lines"), blk_cap = i32(c, "blk_cap"), line_cap = i32(c, "line_cap"),
                dist_cap = i32(c, "dist_cap");
  Buf blines = input(c, "blines", 'i'), cls = input(c, "cls", 'i'), lines = input(c, "lines", 'i'), mask = input(c, "mask", 'b');
  Buf blks = alloc(sizeof(ctd_blk) * (size_t)blk_cap), lout = alloc(sizeof(int32_t) * 8 * (size_t)line_cap),
      dout = alloc(sizeof(double) * 3 * (size_t)dist_cap);
  int32_t nb = -1, nl = -1, nd = -1;
  const int rc = ctd_group_output(blines.as<int32_t>(), cls.as<int32_t>(), n_blk, lines.as<int32_t>(), n_lines, i32(c, "im_w"),
                                  i32(c, "im_h"), mask.as<uint8_t>(), i32(c, "mask_pitch"), blks.as<ctd_blk>(), blk_cap,
                                  lout.as<int32_t>(), line_cap, dout.as<double>(), dist_cap, &nb, &nl, &nd);
  put_i32(r, "rc", rc);
  put_i32(r, "n_blk_out", nb), put_i32(r, "n_lines_out", nl), put_i32(r, "n_dist_out", nd);
  put(r, "blks", 'b', blks.mem.get(), blks.bytes);
  put(r, "lines_out", 'i', lout.mem.get(), 8 * (size_t)line_cap);
  put(r, "dist_out", 'd', dout.mem.get(), 3 * (size_t)dist_cap);
}

void put_boxes(Case& r, int rc, int32_t n, const Buf& boxes, const Buf& scores, int32_t cap) {
  put_i32(r, "rc", rc);
  put_i32(r, "n_out", n);
  put(r, "boxes", 'h', boxes.mem.get(), 8 * (size_t)cap);
  put(r, "scores", 'f', scores.mem.get(), (size_t)cap);
}

void run_db_boxes(const Case& c, Case& r) {
  const int32_t cap = i32(c, "max_candidates");
  Buf prob = input(c, "prob", 'f'), lab_f = input(c, "lab_f", 'i'), st_f = input(c, "st_f", 'i'), lab_b = input(c, "lab_b", 'i'),
      st_b = input(c, "st_b", 'i');
  Buf boxes = alloc(sizeof(int16_t) * 8 * (size_t)cap), scores = alloc(sizeof(float) * (size_t)cap);
  int32_t n = -1;
  const int rc = ctd_db_boxes(prob.as<float>(), lab_f.as<int32_t>(), st_f.as<int32_t>(), i32(c, "n_f"), lab_b.as<int32_t>(),
                              st_b.as<int32_t>(), i32(c, "n_b"), i32(c, "W"), i32(c, "H"), cap, scalar<double>(c, "unclip_ratio", 'd'),
                              boxes.as<int16_t>(), scores.as<float>(), &n);
  put_boxes(r, rc, n, boxes, scores, cap);
}

void run_db_boxes_compact(const Case& c, Case& r) {
  const int32_t cap = i32(c, "max_candidates");
  Buf st_f = input(c, "st_f", 'i'), first_f = input(c, "first_f", 'i'), par_f = input(c, "par_f", 'i'), off_f = input(c, "off_f", 'i'),
      sum_f = input(c, "sum_f", 'd'), st_b = input(c, "st_b", 'i'), first_b = input(c, "first_b", 'i'), par_b = input(c, "par_b", 'i'),
      off_b = input(c, "off_b", 'i'), sum_b = input(c, "sum_b", 'd'), ring_sum = input(c, "ring_sum", 'd'),
      ring_cnt = input(c, "ring_cnt", 'i'), row_lo = input(c, "row_lo", 'i'), row_hi = input(c, "row_hi", 'i');
  Buf boxes = alloc(sizeof(int16_t) * 8 * (size_t)cap), scores = alloc(sizeof(float) * (size_t)cap);
  int32_t n = -1;
  const int rc = ctd_db_boxes_compact(i32(c, "W"), i32(c, "H"), i32(c, "n_f"), st_f.as<int32_t>(), first_f.as<int32_t>(),
                                      par_f.as<int32_t>(), off_f.as<int32_t>(), sum_f.as<double>(), i32(c, "n_b"), st_b.as<int32_t>(),
                                      first_b.as<int32_t>(), par_b.as<int32_t>(), off_b.as<int32_t>(), sum_b.as<double>(),
                                      ring_sum.as<double>(), ring_cnt.as<int32_t>(), row_lo.as<int32_t>(), row_hi.as<int32_t>(), cap,
                                      scalar<double>(c, "unclip_ratio", 'd'), boxes.as<int16_t>(), scores.as<float>(), &n);
  put_boxes(r, rc, n, boxes, scores, cap);
}

void run_topk_colors(const Case& c, Case& r) {
  Buf hist = input(c, "hist", 'l'), colors = alloc(sizeof(double) * 3);
  put_i32(r, "rc", ctd_topk_colors(hist.as<int64_t>(), colors.as<double>()));
  put(r, "colors", 'd', colors.mem.get(), 3);
}

void run_otsu(const Case& c, Case& r) {
  Buf hist = input(c, "hist", 'l');
  put_i32(r, "rc", ctd_otsu_from_hist(hist.as<int64_t>()));
}

void run_inrange(const Case& c, Case& r) {
  Buf lb = alloc(sizeof(int32_t)), ub = alloc(sizeof(int32_t));
  ctd_inrange_bounds(scalar<double>(c, "lo", 'd'), scalar<double>(c, "hi", 'd'), lb.as<int32_t>(), ub.as<int32_t>());
  put_i32(r, "lb", *lb.as<int32_t>()), put_i32(r, "ub", *ub.as<int32_t>());
}

void run_refine_rules(const Case& c, Case& r) {
  Buf hist4 = input(c, "hist4", 'I'), rules = alloc(sizeof(RRule) * 6);
  refine_rules(hist4.as<uint32_t>(), rules.as<RRule>());
  static_assert(sizeof(RRule) == 3 * sizeof(int32_t), "RRule is three int32");
  put(r, "rules", 'i', rules.mem.get(), 18);
}

void run_refine_candidates(const Case& c, Case& r) {
  Buf rules = input(c, "rules", 'i'), sums = input(c, "sums", 'L'), out = alloc(sizeof(RCand) * 4);
  const int n = refine_candidates(rules.as<RRule>(), sums.as<uint64_t>(), scalar<int64_t>(c, "npix", 'l'), out.as<RCand>());
  int32_t rule[4] = {0, 0, 0, 0}, invert[4] = {0, 0, 0, 0};
  uint64_t dist[4] = {0, 0, 0, 0};
  for (int k = 0; k < n && k < 4; ++k) rule[k] = out.as<RCand>()[k].rule, invert[k] = out.as<RCand>()[k].invert, dist[k] = out.as<RCand>()[k].dist;
  put_i32(r, "rc", n);
  put(r, "cand_rule", 'i', rule, 4), put(r, "cand_invert", 'i', invert, 4), put(r, "cand_dist", 'L', dist, 4);
}

void run_host_gather(const Case& c, Case& r) {
  const int32_t n = i32(c, "n");
  Buf sizes = input(c, "sizes", 'L');
  std::vector<Buf> src((size_t)std::max(n, 0));
  size_t total = 0;
  for (int i = 0; i < n; ++i) {
    src[i] = input(c, ("src" + std::to_string(i)).c_str(), 'b');
    total += (size_t)sizes.as<uint64_t>()[i];
  }
  Buf ptrs = find(c, "sizes").present ? alloc(sizeof(void*) * (size_t)n) : Buf();
  for (int i = 0; i < n; ++i) ptrs.as<const void*>()[i] = src[i].mem.get();
  Buf dst = i32(c, "dst_null") ? Buf() : alloc(total);
  static_assert(sizeof(size_t) == sizeof(uint64_t), "sizes are recorded as u64");
  put_i32(r, "rc", ctd_host_gather(dst.mem.get(), ptrs.as<const void*>(), sizes.as<size_t>(), n, i32(c, "threads")));
  put(r, "dst", 'b', dst.mem.get(), dst.bytes);
}

void run_case(const Case& c, Case& r) {
  r.name = c.name, r.entry = c.entry;
  if (c.entry == "ctd_group_output") run_group_output(c, r);
  else if (c.entry == "ctd_db_boxes") run_db_boxes(c, r);
  else if (c.entry == "ctd_db_boxes_compact") run_db_boxes_compact(c, r);
  else if (c.entry == "ctd_topk_colors") run_topk_colors(c, r);
  else if (c.entry == "ctd_otsu_from_hist") run_otsu(c, r);
  else if (c.entry == "ctd_inrange_bounds") run_inrange(c, r);
  else if (c.entry == "refine_rules") run_refine_rules(c, r);
  else if (c.entry == "refine_candidates") run_refine_candidates(c, r);
  else if (c.entry == "ctd_host_gather") run_host_gather(c, r);
  else throw std::runtime_error(c.name + ": unknown entry point " + c.entry);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 4 || (std::strcmp(argv[3], "serial") && (std::strcmp(argv[3], "threads") || argc < 5))) {
    std::fprintf(stderr, "usage: host_replay <cases> <results> serial | threads N\n");
    return 2;
  }
  try {
    const std::vector<Case> cases = read_cases(argv[1]);
    const bool threaded = !std::strcmp(argv[3], "threads");
    const int copies = threaded ? 2 : 1, n_items = (int)cases.size() * copies;
    std::vector<Case> results((size_t)n_items);
    std::atomic<int> failed{0};
    auto item = [&](int i) {
      try {
        run_case(cases[(size_t)(i / copies)], results[(size_t)i]);
        if (threaded) results[(size_t)i].name += i % copies ? "#1" : "#0";
      } catch (const std::exception& e) {
        std::printf("exception in case %s: %s\n", cases[(size_t)(i / copies)].name.c_str(), e.what());
        failed.fetch_add(1);
      }
    };
    if (!threaded) {
      for (int i = 0; i < n_items; ++i) item(i);
    } else {
      const int nt = std::max(1, std::atoi(argv[4]));
      std::atomic<int> next{0};
      auto loop = [&] {
        for (int i = next.fetch_add(1); i < n_items; i = next.fetch_add(1)) item(i);
      };
      std::vector<std::thread> th;
      for (int t = 1; t < nt; ++t) th.emplace_back(loop);
      loop();
      for (auto& t : th) t.join();
    }
    FILE* f = std::fopen(argv[2], "wb");
    if (!f) throw std::runtime_error(std::string("cannot write ") + argv[2]);
    wr(f, "CTDRPLY1", 8);
    for (const Case& r : results) write_case(f, r);
    std::fclose(f);
    std::printf("host_replay: %d cases x %d, %d exceptions\n", (int)cases.size(), copies, failed.load());
    return failed.load() ? 1 : 0;
  } catch (const std::exception& e) {
    std::printf("host_replay: %s\n", e.what());
    return 2;
  }
}
