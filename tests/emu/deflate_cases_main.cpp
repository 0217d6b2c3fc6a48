// The BGZF compressor's host twin (strling_amd/csrc/deflate_core.h: dfl_deflate_host, what strl_bgzf_deflate_host calls) as a
// stand-alone program for AddressSanitizer and UBSan: the shapes of tests/deflate_cases.py, made here, every member inflated
// with zlib and compared, the buffers exact to the byte so that a read or write beside them is seen.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o deflate_cases_main deflate_cases_main.cpp -lz && ./deflate_cases_main
#define STRL_EMU 1
#include <stdio.h>
#include <zlib.h>
#include <string>
#include "../../strling_amd/csrc/deflate_core.h"

using namespace strl;

static uint64_t g_state = 88172645463325252ull;
static uint32_t rnd() { g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17; return (uint32_t)(g_state >> 16); }
static std::vector<uint8_t> random_bytes(size_t n) { std::vector<uint8_t> v(n); for (auto &b : v) b = (uint8_t)rnd(); return v; }
static std::vector<uint8_t> text(size_t n) { std::vector<uint8_t> v(n); for (auto &b : v) b = (uint8_t)"ACGTN"[rnd() % 5]; return v; }
static std::vector<uint8_t> cat(std::initializer_list<std::vector<uint8_t>> parts) { std::vector<uint8_t> v; for (auto &p : parts) v.insert(v.end(), p.begin(), p.end()); return v; }
static std::vector<uint8_t> head(const std::vector<uint8_t> &v, size_t n) { return std::vector<uint8_t>(v.begin(), v.begin() + (ptrdiff_t)n); }

static int g_failed = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { fprintf(stderr, "FAILED %s: ", name.c_str()); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); ++g_failed; return; } } while (0)

static void run(const std::string &name, const std::vector<uint8_t> &data, uint32_t block) {
  // exact-size heap buffers: the sanitizer sees the first byte beside them
  std::vector<uint8_t> in(data), out((size_t)dfl_bound(data.size(), block));
  const size_t nb = (data.size() + block - 1) / block;
  std::vector<uint32_t> csize(nb);
  uint64_t got = 0;
  uint32_t stored = 0;
  const int rc = dfl_deflate_host(in.data(), in.size(), block, out.data(), out.size(), &got, csize.data(), &stored);
  EXPECT(rc == STRL_OK, "rc %d", rc);
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
  EXPECT(dfl_deflate_host(data.data(), data.size(), DFL_MAX_BLOCK, out.data(), need - 1, &got, nullptr, &stored) == STRL_ERR_CAPACITY && clean(0) && got == 77, "capacity");
  EXPECT(dfl_deflate_host(data.data(), data.size(), 0, out.data(), out.size(), &got, nullptr, &stored) == STRL_ERR_ARG && clean(0), "block_bytes 0");
  EXPECT(dfl_deflate_host(data.data(), data.size(), 0xFF01, out.data(), out.size(), &got, nullptr, &stored) == STRL_ERR_ARG && clean(0), "block_bytes 0xFF01");
  EXPECT(dfl_deflate_host(data.data(), data.size(), DFL_MAX_BLOCK, out.data(), out.size(), &got, nullptr, &stored) == STRL_OK && got < data.size() && clean((size_t)got), "dirty buffer");
  EXPECT(dfl_deflate_host(nullptr, 0, DFL_MAX_BLOCK, nullptr, 0, &got, nullptr, &stored) == STRL_OK && got == 0 && stored == 0, "no input");
  printf("ok refusals\n");
}

static void code_lengths() {
  const std::string name = "code_lengths";
  std::unique_ptr<DflWork> W(new DflWork);
  const uint32_t shapes[3][2] = {{286, 15}, {30, 15}, {19, 7}};
  for (auto &s : shapes) {
    std::vector<uint32_t> f(s[0]);
    for (uint32_t i = 0; i < s[0]; ++i) f[i] = i < 2 ? 1u : std::min<uint32_t>(f[i - 1] + f[i - 2], 60000u);
    std::vector<uint8_t> len(s[0]);
    dfl_code_lengths(DflSerial(), *W, f.data(), s[0], s[1], len.data());
    uint64_t kraft = 0;
    for (uint32_t i = 0; i < s[0]; ++i) { EXPECT(len[i] >= 1 && len[i] <= s[1], "length %u", len[i]); kraft += 1ull << (15 - len[i]); }
    EXPECT(kraft == 1ull << 15, "Kraft sum");
  }
  printf("ok code_lengths\n");
}

int main() {
  const uint32_t BLK = DFL_MAX_BLOCK;
  for (size_t n : {0, 1, 3, 4, 5}) run("len" + std::to_string(n), text(n), BLK);
  for (uint32_t b : {1u, 255u, 256u, 257u}) {
    run("block" + std::to_string(b) + "_exact", text(b), b);
    run("block" + std::to_string(b) + "_plus1", text(b + 1), b);
  }
  const std::vector<uint8_t> seq = text(BLK + 1), piece = random_bytes(1000);
  run("full_block", head(seq, BLK), BLK);
  run("full_block_plus1", seq, BLK);
  run("zeros", std::vector<uint8_t>(BLK, 0), BLK);
  run("zeros300", std::vector<uint8_t>(300, 0), BLK);
  run("one_literal", std::vector<uint8_t>(200, 'Q'), BLK);
  {
    std::vector<uint8_t> v;
    for (uint32_t k = 0; v.size() < 300; ++k) { v.push_back((uint8_t)k); v.push_back((uint8_t)(k >> 8)); v.push_back((uint8_t)(0xF0 | (k & 7))); v.push_back(0xE1); }
    v.resize(300);
    run("no_repeated_4gram", v, BLK);
  }
  run("random", random_bytes(BLK), BLK);
  {
    const std::vector<uint8_t> p = random_bytes(600);
    std::vector<uint8_t> v;
    while (v.size() < 20000) v.insert(v.end(), p.begin(), p.end());
    v.resize(20000);
    run("pattern600", v, BLK);
  }
  run("dist32768", cat({piece, text(32768 - 1000), piece, text(100)}), BLK);
  run("dist32769", cat({piece, text(32769 - 1000), piece, text(100)}), BLK);
  run("match_to_the_end", cat({text(700), piece, text(300), head(piece, 600)}), BLK);
  run("match_to_the_end_short", cat({text(300), head(piece, 400), text(100), head(piece, 5)}), BLK);
  {
    const std::vector<uint8_t> two = cat({text(3000), piece});
    run("two_identical_blocks", cat({two, two}), (uint32_t)two.size());
  }
  {
    std::vector<uint32_t> f = {1, 1};
    uint32_t sum = 2;
    while (sum < 4180) { f.push_back(f[f.size() - 1] + f[f.size() - 2]); sum += f.back(); }
    std::vector<uint8_t> v;
    for (size_t s = 0; s < f.size(); ++s) v.insert(v.end(), f[s], (uint8_t)(65 + s));
    for (size_t i = v.size(); i > 1; --i) std::swap(v[i - 1], v[rnd() % i]);
    run("fibonacci_literals", v, BLK);
  }
  refusals();
  code_lengths();
  if (g_failed) { fprintf(stderr, "%d case(s) failed\n", g_failed); return 1; }
  printf("all cases passed\n");
  return 0;
}
