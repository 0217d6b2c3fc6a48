// Host build of the sweep's kernel bodies (strling_amd/csrc/sweep_core.h with STRL_EMU): a workgroup is 256 threads and a
// barrier, the workgroups of a launch run one after the other.  A stand-alone program, so that the CPU suite can run the rule
// itself -- under -fsanitize=address,undefined -- without a device (tests/test_sweep_emu.py).
//
//   sweep_emu FILE
// FILE (text):  n_ref n_bounds n_chunks
//               n_bounds lines   tid beg end                      the queries, sorted by (tid, beg)
//               per chunk        n last
//                 n lines        tid pos flag n_cigar [len op]...   one record each
// Output, per chunk:  "chunk K carry TID MAX unsorted ORD tid ORD" (the carry that leaves the chunk; ORD -1 = none), then one line
//                     "dec BOUND I0 I1 STATUS START STOP" per bound the chunk decided, by bound.
#define STRL_EMU 1
#include <pthread.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <functional>
#include <thread>
#include <vector>
#include "../../strling_amd/csrc/sweep_core.h"

using namespace strl;

static void wait_barrier(void *b) { pthread_barrier_wait(static_cast<pthread_barrier_t *>(b)); }

// the 256 lanes: threads made once, handed one workgroup after the other
struct Lanes {
  pthread_barrier_t go, done, group;
  std::function<void(uint32_t)> job;
  bool stop = false;
  std::vector<std::thread> th;
  Lanes() {
    pthread_barrier_init(&go, nullptr, SW_THREADS + 1);
    pthread_barrier_init(&done, nullptr, SW_THREADS + 1);
    pthread_barrier_init(&group, nullptr, SW_THREADS);
    for (uint32_t t = 0; t < SW_THREADS; ++t)
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
};
static Lanes *lanes;

template <class Body> static void launch(uint32_t blocks, Body body) {
  for (uint32_t b = 0; b < blocks; ++b) {
    SweepShared sh;
    lanes->job = [&, b](uint32_t t) { body(SwGroup{t, b, &lanes->group, wait_barrier}, sh); };
    pthread_barrier_wait(&lanes->go);
    pthread_barrier_wait(&lanes->done);
  }
}

static void put32(std::vector<uint8_t> &o, uint32_t v) { for (int k = 0; k < 4; ++k) o.push_back((uint8_t)(v >> (8 * k))); }
static void put16(std::vector<uint8_t> &o, uint32_t v) { o.push_back((uint8_t)v); o.push_back((uint8_t)(v >> 8)); }

int main(int argc, char **argv) {
  if (argc != 2) { fprintf(stderr, "usage: sweep_emu FILE\n"); return 2; }
  FILE *f = fopen(argv[1], "r");
  if (!f) { perror(argv[1]); return 2; }
  Lanes pool;
  lanes = &pool;
  int n_ref = 0;
  unsigned nb = 0, n_chunks = 0;
  if (fscanf(f, "%d %u %u", &n_ref, &nb, &n_chunks) != 3) return 2;
  std::vector<SweepBound> bounds(nb);
  for (SweepBound &b : bounds) { if (fscanf(f, "%d %d %d", &b.tid, &b.beg, &b.end) != 3) return 2; b.pad = 0; }
  std::vector<uint32_t> dec(nb, SW_OPEN);
  std::vector<SweepDecision> out(nb);
  SweepState S;
  memset(&S, 0, sizeof S);
  S.err_ord[0] = S.err_ord[1] = ~0ull;
  for (int k = 0; k < 2; ++k) { S.carry[k] = SweepCarry{SW_NO_TID, SW_NO_END}; S.last[k] = SweepLast{SW_NO_TID, -1}; }
  uint32_t par = 0;
  unsigned long long ord0 = 0;
  for (unsigned c = 0; c < n_chunks; ++c) {
    unsigned n = 0, last = 0;
    if (fscanf(f, "%u %u", &n, &last) != 2) return 2;
    std::vector<uint8_t> U(64, 0xee);                    // (the records do not start at the buffer's first byte on the device either)
    std::vector<uint32_t> recoff;
    for (unsigned i = 0; i < n; ++i) {
      int tid, pos;
      unsigned flag, n_cig;
      if (fscanf(f, "%d %d %u %u", &tid, &pos, &flag, &n_cig) != 4) return 2;
      recoff.push_back((uint32_t)U.size());
      put32(U, 32u + 2u + 4u * n_cig);                   // block_size: the fixed fields, the name "r", the CIGAR, no SEQ
      put32(U, (uint32_t)tid); put32(U, (uint32_t)pos);
      U.push_back(2); U.push_back(60); put16(U, 0);      // l_read_name, mapq, bin
      put16(U, n_cig); put16(U, flag);
      put32(U, 0); put32(U, 0xffffffffu); put32(U, 0xffffffffu); put32(U, 0);   // l_seq, next refID, next pos, tlen
      U.push_back('r'); U.push_back(0);
      for (unsigned j = 0; j < n_cig; ++j) {
        unsigned len, op;
        if (fscanf(f, "%u %u", &len, &op) != 2) return 2;
        put32(U, (len << 4) | op);
      }
    }
    const uint32_t tiles = (n + SW_THREADS - 1u) / SW_THREADS;
    std::vector<int32_t> tid(n), pos(n), pmax(n);
    std::vector<SweepCarry> tile(tiles);
    SweepParams P{};
    P.U = U.data(); P.recoff = recoff.data(); P.n = n; P.rec_end = (uint32_t)U.size();
    P.ord0 = ord0; P.n_ref = n_ref;
    P.tid = tid.data(); P.pos = pos.data(); P.pmax = pmax.data(); P.tile = tile.data(); P.n_tiles = tiles;
    P.S = &S; P.par = par;
    P.bounds = bounds.data(); P.n_bounds = nb; P.dec = dec.data(); P.out = out.data(); P.last_chunk = last;
    S.n_dec = 0;
    if (n) {
      launch(tiles, [&](const SwGroup &G, SweepShared &sh) { sweep_keys_body(G, P, sh); });
      launch(1, [&](const SwGroup &G, SweepShared &sh) { sweep_tiles_body(G, P, sh); });
    }
    if (n || last) launch((nb + SW_THREADS - 1u) / SW_THREADS, [&](const SwGroup &G, SweepShared &) { sweep_ranges_body(G, P); });
    const SweepCarry C = S.carry[n ? (par ^ 1u) : par];
    printf("chunk %u carry %d %d unsorted %lld tid %lld\n", c, C.tid, C.max_end, (long long)S.err_ord[SW_E_UNSORTED], (long long)S.err_ord[SW_E_TID]);
    std::sort(out.begin(), out.begin() + S.n_dec, [](const SweepDecision &a, const SweepDecision &b) { return a.bound < b.bound; });
    for (uint32_t k = 0; k < S.n_dec; ++k)
      printf("dec %u %u %u %u %llu %llu\n", out[k].bound, out[k].i0, out[k].i1, out[k].status, (unsigned long long)out[k].start, (unsigned long long)out[k].stop);
    if (n) { ord0 += n; par ^= 1u; }
  }
  fclose(f);
  return 0;
}
