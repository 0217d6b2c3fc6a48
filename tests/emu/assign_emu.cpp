// Host build of the kernel bodies of strl_assign_reads_loci_device (strling_amd/csrc/assign_core.h with STRL_EMU): a wave is 64
// threads and a barrier, the waves of a launch run one after the other, a stable host sort stands for the device's radix sort.
// A stand-alone program, so that the CPU suite can run the rule itself -- under -fsanitize=address,undefined -- without a device
// (tests/test_assign_emu.py).
//
//   assign_emu FILE
// FILE (text):  mode n n_loci two_sorts
//               n lines        tid position split unit       a tread ("-": the empty unit)
//               n_loci lines   tid left_most right_most unit a locus
// Output:  "err E" and nothing else when a tread is refused; otherwise "stat GROUPS LOST", then per locus
//          "locus J TOTAL LEFT RIGHT : INDEX ..." (the 32-bit counts and the assigned list), then "marks INDEX ...".
#define STRL_EMU 1
#include <pthread.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <functional>
#include <numeric>
#include <thread>
#include <vector>
#include "../../strling_amd/csrc/assign_core.h"

using namespace strl;

static void wait_barrier(void *b) { pthread_barrier_wait(static_cast<pthread_barrier_t *>(b)); }

// the 64 lanes: threads made once, handed one wave after the other
struct Lanes {
  pthread_barrier_t go, done, group;
  std::function<void(uint32_t)> job;
  bool stop = false;
  std::vector<std::thread> th;
  Lanes() {
    pthread_barrier_init(&go, nullptr, AS_WAVE + 1);
    pthread_barrier_init(&done, nullptr, AS_WAVE + 1);
    pthread_barrier_init(&group, nullptr, AS_WAVE);
    for (uint32_t t = 0; t < AS_WAVE; ++t)
      th.emplace_back([this, t] {
        for (;;) {
          pthread_barrier_wait(&go);
          if (stop) return;
          job(t);
          pthread_barrier_wait(&done);
        }
      });
  }
  ~Lanes() {
    stop = true;
    pthread_barrier_wait(&go);
    for (std::thread &x : th) x.join();
  }
  void run(std::function<void(uint32_t)> f) {
    job = std::move(f);
    pthread_barrier_wait(&go);
    pthread_barrier_wait(&done);
  }
};

static void read_unit(const char *w, char *rep, size_t cap) {
  memset(rep, 0, cap);
  if (strcmp(w, "-")) memcpy(rep, w, std::min(strlen(w), cap));
}

int main(int argc, char **argv) {
  if (argc != 2) { fprintf(stderr, "usage: assign_emu FILE\n"); return 2; }
  FILE *f = fopen(argv[1], "r");
  if (!f) { perror(argv[1]); return 2; }
  int mode = 0, two_sorts = 0;
  unsigned n = 0, nl = 0;
  if (fscanf(f, "%d %u %u %d", &mode, &n, &nl, &two_sorts) != 4) return 2;
  std::vector<strl_tread> treads(n);
  std::vector<AsLocus> loci(nl);
  char w[64];
  for (strl_tread &t : treads) {
    unsigned pos, split;
    memset(&t, 0, sizeof t);
    if (fscanf(f, "%d %u %u %63s", &t.tid, &pos, &split, w) != 4) return 2;
    t.position = pos; t.split = (uint8_t)split;
    read_unit(w, t.repeat, sizeof t.repeat);
  }
  for (AsLocus &l : loci) {
    if (fscanf(f, "%d %u %u %63s", &l.tid, &l.left_most, &l.right_most, w) != 4) return 2;
    read_unit(w, l.rep, 6);
  }
  fclose(f);
  Lanes pool;
  AsStat stat{0u, -1, 0u, 0u};
  AsParams P{};
  P.treads = treads.data(); P.n = n; P.mode = mode; P.loci = loci.data(); P.n_loci = nl; P.stat = &stat;
  for (uint32_t i = 0; i < n; ++i) {
    uint32_t e = 0;
    const int32_t t = as_check_body(P, i, e);
    stat.max_tid = std::max(stat.max_tid, t);
    stat.err |= e;
  }
  if (stat.err) { printf("err %u\n", stat.err); return 0; }
  const uint64_t top = (uint64_t)(uint32_t)(stat.max_tid + 1);
  P.max_tid = stat.max_tid; P.excl = (top << 15) | (7ull << 12); P.composite = two_sorts ? 0 : 1;
  std::vector<uint64_t> key(n), gk(n), skey(n), s_g(n), lkey(nl), slkey(nl), off((size_t)nl + 1);
  std::vector<uint32_t> val(n), sval(n), s_pos(n), owner(n), lval(nl), slval(nl), rng((size_t)nl * 3), cnt((size_t)nl * 3), assigned(n);
  std::vector<uint8_t> s_split(n), mark(n);
  P.key = key.data(); P.val = val.data(); P.gk_in = gk.data();
  for (uint32_t i = 0; i < n; ++i) as_keys_body(P, i);
  auto sort_pairs = [](const std::vector<uint64_t> &k, const std::vector<uint32_t> &v, std::vector<uint64_t> &ok, std::vector<uint32_t> &ov) {
    std::vector<uint32_t> o(k.size());
    std::iota(o.begin(), o.end(), 0u);
    std::stable_sort(o.begin(), o.end(), [&](uint32_t a, uint32_t b) { return k[a] < k[b]; });
    for (size_t i = 0; i < o.size(); ++i) { ok[i] = k[o[i]]; ov[i] = v[o[i]]; }
  };
  sort_pairs(key, val, skey, sval);
  if (!P.composite) {                                    // by position, then by group: as the device does beyond 2^17 references
    for (uint32_t i = 0; i < n; ++i) key[i] = gk[sval[i]];
    val = sval;
    sort_pairs(key, val, skey, sval);
  }
  P.skey = skey.data(); P.sval = sval.data();
  P.s_g = s_g.data(); P.s_pos = s_pos.data(); P.s_split = s_split.data(); P.owner = owner.data();
  for (uint32_t i = 0; i < n; ++i) as_gather_body(P, i);
  P.lkey = lkey.data(); P.lval = lval.data();
  for (uint32_t j = 0; j < nl; ++j) as_lkeys_body(P, j);
  sort_pairs(lkey, lval, slkey, slval);
  P.slkey = slkey.data(); P.slval = slval.data();
  P.p0 = rng.data(); P.p1 = P.p0 + nl; P.ge = P.p1 + nl;
  P.cnt = cnt.data(); P.off = off.data(); P.assigned = assigned.data(); P.mark = mark.data();
  for (uint32_t k = 0; k < nl; ++k) as_ranges_body(P, k);
  AsShared sh;
  for (uint32_t k = 0; k < nl; ++k) pool.run([&, k](uint32_t t) { as_take_body(AsWave{t, &sh, &pool.group, wait_barrier}, P, k); });
  std::vector<uint64_t> ssh(AS_SCAN_MAX);
  pool.run([&](uint32_t t) { as_scan_body(AsBlock{t, AS_WAVE, &pool.group, wait_barrier}, P, ssh.data()); });
  for (uint32_t j = 0; j < nl; ++j) pool.run([&, j](uint32_t t) { as_fill_body(AsWave{t, &sh, &pool.group, wait_barrier}, P, j); });
  for (uint32_t i = 0; i < n; ++i) as_marks_body(P, i);
  printf("stat %u %u\n", stat.n_groups, stat.n_lost);
  for (uint32_t j = 0; j < nl; ++j) {
    printf("locus %u %u %u %u :", j, cnt[j], cnt[(size_t)nl + j], cnt[2 * (size_t)nl + j]);
    for (uint64_t q = off[j]; q < off[(size_t)j + 1]; ++q) printf(" %u", assigned[q]);
    printf("\n");
  }
  printf("marks");
  for (uint32_t i = 0; i < n; ++i) if (mark[i]) printf(" %u", i);
  printf("\n");
  for (uint32_t i = 0; i < n; ++i)
    if (mark[i] && treads[i].split != STRL_SOFT_TAKEN) return 3;       // the mark column and the treads' own column agree
  return 0;
}
