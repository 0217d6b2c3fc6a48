// The dense rule of the BGZF compressor (strling_amd/csrc/deflate_core.h: DflDense) as a stand-alone program for AddressSanitizer
// and UBSan: shapes made for its chains, ring and lazy parse in buffers exact to the byte, every member inflated with zlib and
// compared.  Every shape runs twice: as the host twin (a team of one that inserts in position order) and as the kernel's side of
// the rule -- the lanes' loops, with the backward scan over a batch's hashes and the insert behind the search -- on one thread;
// the two must write the same bytes.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o deflate_dense_main deflate_dense_main.cpp -lz && ./deflate_dense_main
#define STRL_EMU 1
#include <stdio.h>
#include <zlib.h>
#include <string>
#include "../../strling_amd/csrc/deflate_core.h"

using namespace strl;

// the kernel's side of the rule on one thread: nothing in it relies on the order the positions of a batch are visited in
struct LanesOnOneThread : DflSerial {
  static constexpr bool IN_ORDER = false;
};

static uint64_t g_state = 88172645463325252ull;
static uint32_t rnd() { g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17; return (uint32_t)(g_state >> 16); }
static std::vector<uint8_t> random_bytes(size_t n) { std::vector<uint8_t> v(n); for (auto &b : v) b = (uint8_t)rnd(); return v; }
static std::vector<uint8_t> text(size_t n) { std::vector<uint8_t> v(n); for (auto &b : v) b = (uint8_t)"ACGTN"[rnd() % 5]; return v; }
static std::vector<uint8_t> cat(std::initializer_list<std::vector<uint8_t>> parts) { std::vector<uint8_t> v; for (auto &p : parts) v.insert(v.end(), p.begin(), p.end()); return v; }
static std::vector<uint8_t> head(const std::vector<uint8_t> &v, size_t n) { return std::vector<uint8_t>(v.begin(), v.begin() + (ptrdiff_t)n); }
static std::vector<uint8_t> times(const std::vector<uint8_t> &v, size_t n) { std::vector<uint8_t> r; while (r.size() < n) r.insert(r.end(), v.begin(), v.end()); r.resize(n); return r; }

static int g_failed = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { fprintf(stderr, "FAILED %s: ", name.c_str()); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); ++g_failed; return; } } while (0)

static void run(const std::string &name, const std::vector<uint8_t> &data, uint32_t block) {
  // exact-size heap buffers: the sanitizer sees the first byte beside them
  std::vector<uint8_t> in(data), out((size_t)dfl_bound(data.size(), block)), lanes(out.size());
  const size_t nb = (data.size() + block - 1) / block;
  std::vector<uint32_t> csize(nb), csize_lanes(nb);
  uint64_t got = 0, got_lanes = 0;
  uint32_t stored = 0, stored_lanes = 0;
  int rc = dfl_deflate_host_mode(STRL_DEFLATE_DENSE, in.data(), in.size(), block, out.data(), out.size(), &got, csize.data(), &stored);
  EXPECT(rc == STRL_OK, "rc %d", rc);
  rc = dfl_deflate_host_as<DflDense, LanesOnOneThread>(in.data(), in.size(), block, lanes.data(), lanes.size(), &got_lanes, csize_lanes.data(), &stored_lanes);
  EXPECT(rc == STRL_OK && got_lanes == got && stored_lanes == stored && csize_lanes == csize && (!got || !memcmp(lanes.data(), out.data(), (size_t)got)),
         "the lanes' side of the rule writes other bytes: rc %d, %llu / %llu bytes", rc, (unsigned long long)got_lanes, (unsigned long long)got);
  uint64_t at = 0;
  uint32_t seen_stored = 0;
  for (size_t k = 0; k < nb; ++k) {
    const uint8_t *m = out.data() + at;
    const uint32_t sz = csize[k], n = (uint32_t)std::min<size_t>(block, data.size() - k * block);
    EXPECT(at + sz <= got && sz >= 26 && sz <= n + 31 && sz <= 65536, "member %zu: size %u", k, sz);
    EXPECT((uint32_t)(m[16] | m[17] << 8) == sz - 1, "member %zu: BSIZE", k);
    seen_stored += ((m[18] >> 1) & 3) == 0;
    std::vector<uint8_t> back(n + 1);
    z_stream zs;
    memset(&zs, 0, sizeof zs);
    EXPECT(inflateInit2(&zs, -15) == Z_OK, "inflateInit2");
    zs.next_in = const_cast<uint8_t *>(m + 18); zs.avail_in = sz - 26;
    zs.next_out = back.data(); zs.avail_out = n + 1;
    const int zr = inflate(&zs, Z_FINISH);
    const uLong total = zs.total_out;
    const uInt left = zs.avail_in;
    inflateEnd(&zs);
    EXPECT(zr == Z_STREAM_END && total == n && left == 0, "member %zu: inflate %d, %lu of %u bytes, %u unread", k, zr, total, n, left);
    EXPECT(!memcmp(back.data(), data.data() + k * block, n), "member %zu: bytes", k);
    uint32_t crc, isz;
    memcpy(&crc, m + sz - 8, 4); memcpy(&isz, m + sz - 4, 4);
    EXPECT(crc == (uint32_t)crc32(crc32(0, nullptr, 0), data.data() + k * block, n) && isz == n, "member %zu: CRC-32 / ISIZE", k);
    at += sz;
  }
  EXPECT(at == got && seen_stored == stored, "%llu bytes in members, %llu reported; stored %u / %u", (unsigned long long)at, (unsigned long long)got, seen_stored, stored);
  printf("ok %-26s %7zu bytes, block %5u -> %7llu bytes, %u stored\n", name.c_str(), data.size(), block, (unsigned long long)got, stored);
}

static void refusals() {
  const std::string name = "refusals";
  const std::vector<uint8_t> data = text(100000);
  const uint64_t need = dfl_bound(data.size(), DFL_MAX_BLOCK);
  std::vector<uint8_t> out((size_t)need + 64, 0xA5);
  uint64_t got = 77;
  uint32_t stored = 77;
  auto clean = [&](size_t from) { for (size_t i = from; i < out.size(); ++i) if (out[i] != 0xA5) return false; return true; };
  const int M = STRL_DEFLATE_DENSE;
  EXPECT(dfl_deflate_host_mode(M, data.data(), data.size(), DFL_MAX_BLOCK, out.data(), need - 1, &got, nullptr, &stored) == STRL_ERR_CAPACITY && clean(0) && got == 77, "capacity");
  EXPECT(dfl_deflate_host_mode(M, data.data(), data.size(), 0, out.data(), out.size(), &got, nullptr, &stored) == STRL_ERR_ARG && clean(0), "block_bytes 0");
  EXPECT(dfl_deflate_host_mode(M, data.data(), data.size(), 0xFF01, out.data(), out.size(), &got, nullptr, &stored) == STRL_ERR_ARG && clean(0), "block_bytes 0xFF01");
  EXPECT(dfl_deflate_host_mode(2, data.data(), data.size(), DFL_MAX_BLOCK, out.data(), out.size(), &got, nullptr, &stored) == STRL_ERR_ARG && clean(0), "mode 2");
  EXPECT(dfl_deflate_host_mode(-1, data.data(), data.size(), DFL_MAX_BLOCK, out.data(), out.size(), &got, nullptr, &stored) == STRL_ERR_ARG && clean(0), "mode -1");
  EXPECT(dfl_deflate_host_mode(M, data.data(), data.size(), DFL_MAX_BLOCK, out.data(), out.size(), &got, nullptr, &stored) == STRL_OK && got < data.size() && clean((size_t)got), "dirty buffer");
  EXPECT(dfl_deflate_host_mode(M, nullptr, 0, DFL_MAX_BLOCK, nullptr, 0, &got, nullptr, &stored) == STRL_OK && got == 0 && stored == 0, "no input");
  printf("ok refusals\n");
}

int main() {
  const uint32_t BLK = DFL_MAX_BLOCK, W = DflDense::WINDOW, RING = DflDense::RING;
  for (size_t n : {0, 1, 3, 4, 5}) run("len" + std::to_string(n), text(n), BLK);
  for (uint32_t b : {1u, 255u, 256u, 257u}) {
    run("block" + std::to_string(b) + "_exact", text(b), b);
    run("block" + std::to_string(b) + "_plus1", text(b + 1), b);
  }
  const std::vector<uint8_t> seq = text(BLK + 1), piece = random_bytes(1000);
  run("full_block", head(seq, BLK), BLK);                                                // every chain at full depth
  run("full_block_plus1", seq, BLK);
  run("zeros", std::vector<uint8_t>(BLK, 0), BLK);                                      // one chain of 65 k entries, distance 1
  run("zeros300", std::vector<uint8_t>(300, 0), BLK);
  run("period4", times({'a', 'b', 'c', 'd'}, BLK), BLK);                                // one chain per residue, distance 4
  run("period4_short", times({'a', 'b', 'c', 'd'}, 400), BLK);
  run("random", random_bytes(BLK), BLK);
  run("pattern600", times(random_bytes(600), 20000), BLK);
  run("dist_window", cat({piece, text(W - 1000), piece, text(100)}), BLK);              // a match at distance W exactly
  run("dist_window_plus1", cat({piece, text(W + 1 - 1000), piece, text(100)}), BLK);
  run("dist_ring", cat({piece, text(RING - 1000), piece, text(RING - 1000), piece}), BLK);   // positions that share ring slots, block > 2 W
  run("match_to_the_end", cat({text(700), piece, text(300), head(piece, 600)}), BLK);
  run("match_to_the_end_short", cat({text(300), head(piece, 400), text(100), head(piece, 5)}), BLK);
  run("lazy_at_the_end", cat({text(300), head(piece, 8), text(50), std::vector<uint8_t>(piece.begin() + 1, piece.begin() + 20), text(40), head(piece, 5)}), BLK);
  {
    const std::vector<uint8_t> two = cat({text(3000), piece});
    run("two_identical_blocks", cat({two, two}), (uint32_t)two.size());
  }
  {
    std::vector<uint8_t> v;                                                             // 600 blocks of 256, every odd one its predecessor's copy
    for (int k = 0; k < 300; ++k) { const std::vector<uint8_t> t = text(256); v.insert(v.end(), t.begin(), t.end()); v.insert(v.end(), t.begin(), t.end()); }
    run("small_blocks", v, 256);
  }
  {
    std::vector<uint8_t> v = text(40000);                                               // a block behind a longer one: slots of the ring left over
    const std::vector<uint8_t> t = text(300);
    v.insert(v.end(), t.begin(), t.end());
    run("short_behind_long", v, 40000);
  }
  refusals();
  if (g_failed) { fprintf(stderr, "%d case(s) failed\n", g_failed); return 1; }
  printf("all cases passed\n");
  return 0;
}
