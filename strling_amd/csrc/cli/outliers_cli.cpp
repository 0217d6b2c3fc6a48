// outliers_cli.cpp -- `strling outliers`: the reference's fifth stage, scripts/strling-outliers.py ("the script"; line numbers
// below cite it), with its statistics on the device (csrc/outliers.hip through the C ABI).
//
// Host: argument parsing (argparse's messages and exit codes), glob(3) expansion, the input files on up to 16 threads, locus
// interning in the pivot's order, sum_str_log with the host libm (as numpy), and the text of the outputs (Python repr, '.2g',
// pandas Int64 / na_rep rules).  Device: depth medians, Huber per locus, z / p / BH, the output order.  Everything that can be
// wrong with the arguments or the input files is found before the device is opened.
#include <errno.h>
#include <glob.h>
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <map>
#include <set>
#include <string>
#include <string_view>
#include <thread>
#include <unordered_map>
#include <vector>
#include "../../../include/strling_amd.h"

namespace {

const double NaN = __builtin_nan("");
constexpr int32_t INT_NA = INT32_MIN;      // a pandas Int64 <NA> cell

[[noreturn]] void die(int code, const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vfprintf(stderr, fmt, ap);
  va_end(ap);
  fputc('\n', stderr);
  exit(code);
}

const char *USAGE =
    "usage: strling outliers [-h] --genotypes GENOTYPES [GENOTYPES ...] --unplaced UNPLACED [UNPLACED ...] [--out OUT]\n"
    "                        [--control CONTROL] [--emit EMIT] [--slop SLOP] [--min_clips MIN_CLIPS] [--min_size MIN_SIZE]\n"
    "                        [--debug] [-v]\n";

const char *HELP =
    "\nRead STRling output and look for individuals that are outliers at STR loci\n\n"
    "optional arguments:\n"
    "  -h, --help            show this help message and exit\n"
    "  --genotypes GENOTYPES [GENOTYPES ...]\n"
    "                        -genotype.txt files for all samples produced by STRling. Optionally takes glob patterns as strings.\n"
    "  --unplaced UNPLACED [UNPLACED ...]\n"
    "                        -unplaced.txt files for all samples produced by STRling. Contains the number of unassigned STR reads\n"
    "                        for each repeat unit. Optionally takes glob patterns as strings.\n"
    "  --out OUT             Prefix for all output files (suffix will be STRs.tsv) (default: )\n"
    "  --control CONTROL     Input file for median and standard deviation estimates at each locus from a set of control samples.\n"
    "                        This file can be produced by this script using the emit option. If this option is not set, all\n"
    "                        samples in the current batch will be used as controls by default.\n"
    "  --emit EMIT           Output file for median and standard deviation estimates at each locus (tsv).\n"
    "  --slop SLOP           Merge loci that are within this many bp of each other and have the same repeat unit.\n"
    "  --min_clips MIN_CLIPS\n"
    "                        In the individual sample files, only report loci with at least many soft-cliped reads in that sample.\n"
    "  --min_size MIN_SIZE   In the individual sample files, only report loci with at least this allele2_est size in that sample.\n"
    "  --debug               Add column to output for estimation method\n"
    "  -v                    (this build) phase timings on stderr; changes no output file\n";

[[noreturn]] void arg_error(const std::string &msg) {
  fputs(USAGE, stderr);
  die(2, "strling outliers: error: %s", msg.c_str());
}

struct Args {
  std::vector<std::string> genotypes, unplaced;
  std::string out, control, emit;
  long slop = 50, min_clips = 0, min_size = 0;
  bool debug = false, verbose = false, have_g = false, have_u = false;
};

long parse_int_arg(const std::string &opt, const std::string &v) {
  char *e = nullptr;
  errno = 0;
  const long x = strtol(v.c_str(), &e, 10);
  if (v.empty() || *e || errno) arg_error("argument " + opt + ": invalid int value: '" + v + "'");
  return x;
}

Args parse_args(int argc, char **argv) {
  Args a;
  std::vector<std::string> unknown;
  for (int i = 2; i < argc;) {
    std::string k = argv[i], v;
    bool has_eq = false;
    if (k.rfind("--", 0) == 0 && k.find('=') != std::string::npos) { v = k.substr(k.find('=') + 1); k = k.substr(0, k.find('=')); has_eq = true; }
    auto value = [&]() -> std::string {
      if (has_eq) { ++i; return v; }
      if (i + 1 >= argc || (argv[i + 1][0] == '-' && argv[i + 1][1])) arg_error("argument " + k + ": expected one argument");
      i += 2;
      return argv[i - 1];
    };
    if (k == "-h" || k == "--help") { fputs(USAGE, stdout); fputs(HELP, stdout); exit(0); }
    if (k == "--genotypes" || k == "--unplaced") {
      std::vector<std::string> &dst = k == "--genotypes" ? a.genotypes : a.unplaced;
      (k == "--genotypes" ? a.have_g : a.have_u) = true;
      dst.clear();
      if (has_eq) { dst.push_back(v); ++i; }
      else {
        ++i;
        while (i < argc && !(argv[i][0] == '-' && argv[i][1])) dst.push_back(argv[i++]);
      }
      if (dst.empty()) arg_error("argument " + k + ": expected at least one argument");
    } else if (k == "--out") a.out = value();
    else if (k == "--control") a.control = value();
    else if (k == "--emit") a.emit = value();
    else if (k == "--slop") a.slop = parse_int_arg(k, value());
    else if (k == "--min_clips") a.min_clips = parse_int_arg(k, value());
    else if (k == "--min_size") a.min_size = parse_int_arg(k, value());
    else if (k == "--debug") { a.debug = true; ++i; }
    else if (k == "-v") { a.verbose = true; ++i; }
    else { unknown.push_back(argv[i]); ++i; }
  }
  std::string req;
  if (!a.have_g) req += "--genotypes";
  if (!a.have_u) req += std::string(req.empty() ? "" : ", ") + "--unplaced";
  if (!req.empty()) arg_error("the following arguments are required: " + req);
  if (!unknown.empty()) {
    std::string u;
    for (const auto &x : unknown) u += (u.empty() ? "" : " ") + x;
    arg_error("unrecognized arguments: " + u);
  }
  return a;
}

// glob_list :170-175, each pattern through glob(3) (sorted; the script's order is the file system's)
std::vector<std::string> glob_list(const std::vector<std::string> &pats) {
  std::vector<std::string> out;
  for (const auto &p : pats) {
    glob_t g{};
    if (glob(p.c_str(), 0, nullptr, &g) == 0)
      for (size_t k = 0; k < g.gl_pathc; ++k) out.push_back(g.gl_pathv[k]);
    globfree(&g);
  }
  return out;
}

std::string get_sample(const std::string &path) {       // :64-67
  const size_t sl = path.rfind('/');
  const std::string base = sl == std::string::npos ? path : path.substr(sl + 1);
  const size_t d = base.rfind('-');
  return d == std::string::npos ? base : base.substr(0, d);
}

bool read_file(const std::string &path, std::string &buf) {
  FILE *f = fopen(path.c_str(), "rb");
  if (!f) return false;
  buf.clear();
  char tmp[1 << 16];
  size_t n;
  while ((n = fread(tmp, 1, sizeof tmp, f)) > 0) buf.append(tmp, n);
  fclose(f);
  return true;
}

// whitespace-separated fields of one line (read_csv delim_whitespace: runs of blanks are one separator)
void split_ws(std::string_view line, std::vector<std::string_view> &f) {
  f.clear();
  size_t i = 0;
  while (i < line.size()) {
    while (i < line.size() && (line[i] == ' ' || line[i] == '\t' || line[i] == '\r')) ++i;
    if (i >= line.size()) break;
    size_t j = i;
    while (j < line.size() && line[j] != ' ' && line[j] != '\t' && line[j] != '\r') ++j;
    f.push_back(line.substr(i, j - i));
    i = j;
  }
}

bool is_na(std::string_view t) {     // pandas' default NA strings
  static const char *na[] = {"", "nan", "NaN", "NA", "N/A", "NULL", "null", "n/a", "-nan", "-NaN", "#N/A", "<NA>", "None",
                             "1.#QNAN", "#NA", "-1.#QNAN", "-1.#IND", "1.#IND"};
  for (const char *s : na) if (t == s) return true;
  return false;
}

double to_num(std::string_view t) {
  if (is_na(t)) return NaN;
  char b[64];
  const size_t n = std::min(t.size(), sizeof b - 1);
  memcpy(b, t.data(), n);
  b[n] = 0;
  char *e = nullptr;
  const double v = strtod(b, &e);
  return (e && *e == 0) ? v : NaN;
}

bool is_int_token(std::string_view t) {
  if (!t.empty() && (t[0] == '+' || t[0] == '-')) t.remove_prefix(1);
  if (t.empty()) return false;
  for (char ch : t) if (ch < '0' || ch > '9') return false;
  return true;
}

int32_t to_int(std::string_view t) {
  const double v = to_num(t);
  return v != v ? INT_NA : (int32_t)v;
}

// ---------------------------------------------------------------- number text

// Python repr(float): the shortest digits that read back to x; fixed notation for exponents -4 .. 15, else d.ddde+XX
void py_repr(double x, std::string &o) {
  if (x != x) { o += "nan"; return; }
  if (isinf(x)) { o += x < 0 ? "-inf" : "inf"; return; }
  if (x == 0) { o += signbit(x) ? "-0.0" : "0.0"; return; }
  char b[40];
  int prec = 1;
  for (; prec < 17; ++prec) {
    snprintf(b, sizeof b, "%.*e", prec - 1, x);
    if (strtod(b, nullptr) == x) break;
  }
  snprintf(b, sizeof b, "%.*e", prec - 1, x);
  // b = [-]d[.ddd]e[+-]XX
  std::string digits;
  const char *p = b;
  const bool neg = *p == '-';
  if (neg) ++p;
  for (; *p && *p != 'e'; ++p) if (*p != '.') digits += *p;
  const int e10 = atoi(p + 1);
  while (digits.size() > 1 && digits.back() == '0') digits.pop_back();
  if (neg) o += '-';
  if (e10 >= -4 && e10 < 16) {
    if (e10 >= 0) {
      const size_t ip = (size_t)e10 + 1;
      if (digits.size() <= ip) { o += digits; o.append(ip - digits.size(), '0'); o += ".0"; }
      else { o.append(digits, 0, ip); o += '.'; o.append(digits, ip, std::string::npos); }
    } else {
      o += "0.";
      o.append((size_t)(-e10 - 1), '0');
      o += digits;
    }
  } else {
    o += digits[0];
    if (digits.size() > 1) { o += '.'; o.append(digits, 1, std::string::npos); }
    char eb[8];
    snprintf(eb, sizeof eb, "e%c%02d", e10 < 0 ? '-' : '+', abs(e10));
    o += eb;
  }
}

// a float64 cell of to_csv: repr, NaN as na_rep 'NaN'
void cell_float(double x, std::string &o) {
  if (x != x) o += "NaN";
  else py_repr(x, o);
}

// repr(np.round(x, 1)) = repr(rint(10 x) / 10): the decimal k / 10 itself, k = rint(10 x) (:456)
void cell_round1(double x, std::string &o) {
  if (x != x) { o += "NaN"; return; }
  const double k = rint(x * 10.0);
  const double v = k / 10.0;
  if (!(fabs(k) < 1e15)) { py_repr(v, o); return; }
  long long ki = (long long)k;
  if (ki == 0) { o += signbit(v) ? "-0.0" : "0.0"; return; }
  if (ki < 0) { o += '-'; ki = -ki; }
  char b[32];
  snprintf(b, sizeof b, "%lld.%lld", ki / 10, ki % 10);
  o += b;
}

// format(x, '.2g') (:453-455)
void cell_g2(double x, std::string &o) {
  if (x != x) { o += "nan"; return; }
  if (isinf(x)) { o += x < 0 ? "-inf" : "inf"; return; }
  char b[32];
  snprintf(b, sizeof b, "%.2g", x);
  o += b;
}

void cell_int(int64_t v, std::string &o) {
  if (v == INT_NA) { o += "NaN"; return; }
  char b[24];
  snprintf(b, sizeof b, "%lld", (long long)v);
  o += b;
}

// ---------------------------------------------------------------- input

struct Cell {            // one -genotype.txt row
  uint32_t key_off, key_len, chrom_len;
  uint32_t locus;        // interned id, later the locus' rank
  double a1, a2, depth, ssc;
  int32_t ints[5];       // spanning_reads, spanning_pairs, left_clips, right_clips, unplaced_pairs
  int32_t left, right;
};

struct Sample {
  std::string name, gpath, upath;
  std::string keys;                       // "chrom-left-right-repeatunit" of every row, back to back
  std::vector<Cell> cells;
  std::vector<std::pair<std::string, double>> unplaced;
  bool unplaced_float = false;
  std::string err;
};

const char *GCOLS[] = {"chrom", "left", "right", "repeatunit", "allele1_est", "allele2_est", "spanning_reads", "spanning_pairs",
                       "left_clips", "right_clips", "unplaced_pairs", "depth", "sum_str_counts"};
constexpr int NG = 13;

void parse_sample(Sample &s) {
  std::string buf;
  if (!read_file(s.upath, buf)) { s.err = "[Errno 2] No such file or directory: '" + s.upath + "'"; return; }
  std::vector<std::string_view> f;
  size_t pos = 0;
  bool any = false;
  while (pos < buf.size()) {                 // parse_unplaced :69-79 (no header)
    size_t e = buf.find('\n', pos);
    if (e == std::string::npos) e = buf.size();
    split_ws(std::string_view(buf).substr(pos, e - pos), f);
    pos = e + 1;
    if (f.empty()) continue;
    any = true;
    const std::string_view c = f.size() > 1 ? f[1] : std::string_view();
    s.unplaced_float |= !is_int_token(c);
    s.unplaced.emplace_back(std::string(f[0]), f.size() > 1 ? to_num(c) : NaN);
  }
  if (!any) { s.err = "ERROR: file " + s.upath + " was empty.\n"; return; }
  if (!read_file(s.gpath, buf)) { s.err = "[Errno 2] No such file or directory: '" + s.gpath + "'"; return; }
  pos = 0;
  int col[NG];
  bool head = false;
  while (pos < buf.size()) {                 // parse_genotypes :81-96
    size_t e = buf.find('\n', pos);
    if (e == std::string::npos) e = buf.size();
    split_ws(std::string_view(buf).substr(pos, e - pos), f);
    pos = e + 1;
    if (f.empty()) continue;
    if (!head) {
      head = true;
      for (int k = 0; k < NG; ++k) {
        col[k] = -1;
        for (size_t j = 0; j < f.size(); ++j)
          if (f[j] == GCOLS[k] || (k == 0 && f[j] == "#chrom")) { col[k] = (int)j; break; }
        if (col[k] < 0) { s.err = std::string("KeyError: '") + GCOLS[k] + "' (no such column in " + s.gpath + ")"; return; }
      }
      continue;
    }
    auto fld = [&](int k) { return (size_t)col[k] < f.size() ? f[(size_t)col[k]] : std::string_view(); };
    Cell c{};
    c.key_off = (uint32_t)s.keys.size();
    s.keys.append(fld(0)); s.keys += '-';
    c.chrom_len = (uint32_t)fld(0).size();
    s.keys.append(fld(1)); s.keys += '-';
    s.keys.append(fld(2)); s.keys += '-';
    s.keys.append(fld(3));
    c.key_len = (uint32_t)(s.keys.size() - c.key_off);
    c.left = to_int(fld(1));
    c.right = to_int(fld(2));
    c.a1 = to_num(fld(4));
    c.a2 = to_num(fld(5));
    for (int k = 0; k < 5; ++k) c.ints[k] = to_int(fld(6 + k));
    c.depth = to_num(fld(11));
    c.ssc = to_num(fld(12));
    s.cells.push_back(c);
  }
  if (!head) { s.err = "ERROR: file " + s.gpath + " was empty.\n"; return; }
  if (s.cells.empty()) { s.err = "ERROR: file " + s.gpath + " contained 0 loci.\n"; return; }
}

template <class F>
void parallel_for(size_t n, int threads, F fn) {
  std::atomic<size_t> next{0};
  std::vector<std::thread> pool;
  const int T = (int)std::max<size_t>(1, std::min<size_t>((size_t)threads, n));
  for (int t = 0; t < T; ++t)
    pool.emplace_back([&]() { for (size_t i; (i = next.fetch_add(1)) < n;) fn(i); });
  for (auto &th : pool) th.join();
}

int host_threads() {
  const unsigned hc = std::thread::hardware_concurrency();
  return (int)std::max(1u, std::min(hc ? hc : 1u, 16u));
}

struct Timer {
  bool on;
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now(), last = t0;
  std::vector<std::pair<std::string, double>> laps;
  void lap(const char *what) {
    const auto now = std::chrono::steady_clock::now();
    laps.emplace_back(what, std::chrono::duration<double>(now - last).count());
    last = now;
  }
};

#define CK(call)                                                                         \
  do {                                                                                   \
    if ((call) != STRL_OK) die(1, "[strling] %s: %s", #call, strl_last_error());         \
  } while (0)

bool write_text(const std::string &path, const std::string &text) {
  FILE *f = fopen(path.c_str(), "wb");
  if (!f) return false;
  const bool ok = fwrite(text.data(), 1, text.size(), f) == text.size();
  return fclose(f) == 0 && ok;
}

struct Control {
  std::unordered_map<std::string, std::pair<double, double>> est;
  std::vector<std::string> loci;          // in file order, null_locus_counts excluded
  double null_mu = NaN, null_sd = NaN;
};

// parse_controls :98-113 (read_csv index_col=0, delim_whitespace)
Control read_control(const std::string &path) {
  Control c;
  std::string buf;
  if (!read_file(path, buf)) die(1, "FileNotFoundError: [Errno 2] No such file or directory: '%s'", path.c_str());
  std::vector<std::string_view> f;
  size_t pos = 0;
  bool head = false, have_null = false;
  while (pos < buf.size()) {
    size_t e = buf.find('\n', pos);
    if (e == std::string::npos) e = buf.size();
    split_ws(std::string_view(buf).substr(pos, e - pos), f);
    pos = e + 1;
    if (f.empty()) continue;
    if (!head) {
      head = true;
      std::string names = "[";
      for (size_t j = 1; j < f.size(); ++j) names += std::string(j > 1 ? ", '" : "'") + std::string(f[j]) + "'";
      names += "]";
      if (!(f.size() >= 3 && (f[1] == "mu" || f[1] == "median") && (f[2] == "sd" || f[2] == "SD")))
        die(1, "ValueError: The column names in the control file don't look right, expecting columns named median, SD or mu, sd. "
               "Column names are %s. Check the file: %s", names.c_str(), path.c_str());
      continue;
    }
    const std::string loc(f[0]);
    const double mu = f.size() > 1 ? to_num(f[1]) : NaN, sd = f.size() > 2 ? to_num(f[2]) : NaN;
    if (loc == "null_locus_counts") { c.null_mu = mu; c.null_sd = sd; have_null = true; continue; }
    if (!c.est.count(loc)) c.loci.push_back(loc);
    c.est[loc] = {mu, sd};
  }
  if (!head) die(1, "pandas.errors.EmptyDataError: No columns to parse from file");
  if (!have_null) die(1, "KeyError: 'null_locus_counts'");
  return c;
}

}  // namespace

int outliers_main(int argc, char **argv) {
  const Args a = parse_args(argc, argv);
  Timer tm{a.verbose};
  const int T = host_threads();

  // ---- files and samples :187-208
  const std::vector<std::string> gfiles = glob_list(a.genotypes), ufiles = glob_list(a.unplaced);
  std::map<std::string, std::string> gby, uby;
  for (const auto &f : gfiles) gby[get_sample(f)] = f;
  for (const auto &f : ufiles) uby[get_sample(f)] = f;
  {
    std::set<std::string> missing;
    for (const auto &kv : gby) if (!uby.count(kv.first)) missing.insert(kv.first);
    for (const auto &kv : uby) if (!gby.count(kv.first)) missing.insert(kv.first);
    if (!missing.empty()) {
      std::string m;
      for (const auto &s : missing) m += (m.empty() ? "" : " ") + s;
      die(1, "ERROR: One or more files are missing for sample(s): %s", m.c_str());
    }
  }
  if (ufiles.empty()) die(1, "ValueError: No objects to concatenate");
  fprintf(stderr, "Reading input files for %zu samples\n", gby.size());
  if (gby.size() < 2 && a.control.empty())
    fputs("WARNING: Only 1 sample and no control file provided, so outlier scores and p-values will not be generated.", stderr);

  std::vector<Sample> S(gby.size());
  {
    size_t k = 0;
    for (const auto &kv : gby) { S[k].name = kv.first; S[k].gpath = kv.second; S[k].upath = uby[kv.first]; ++k; }
  }
  const size_t NS = S.size();
  parallel_for(NS, T, [&](size_t i) { parse_sample(S[i]); });
  for (const auto &s : S) if (!s.err.empty()) die(1, "%s", s.err.c_str());
  Control ctl;
  if (!a.control.empty()) ctl = read_control(a.control);

  // ---- intern the locus keys; the pivot's order (:255) is the sorted order of the strings
  std::unordered_map<std::string_view, uint32_t> ids;
  std::vector<std::string_view> keys;
  std::vector<std::pair<uint32_t, uint32_t>> first;      // (sample, cell) of a locus' first row: chrom / left / right / unit
  for (size_t s = 0; s < NS; ++s)
    for (size_t j = 0; j < S[s].cells.size(); ++j) {
      Cell &c = S[s].cells[j];
      const std::string_view k(S[s].keys.data() + c.key_off, c.key_len);
      auto it = ids.find(k);
      if (it == ids.end()) { it = ids.emplace(k, (uint32_t)keys.size()).first; keys.push_back(k); first.emplace_back((uint32_t)s, (uint32_t)j); }
      c.locus = it->second;
    }
  const size_t LA = keys.size();
  std::vector<uint32_t> by_rank(LA), rank(LA);
  for (size_t i = 0; i < LA; ++i) by_rank[i] = (uint32_t)i;
  std::sort(by_rank.begin(), by_rank.end(), [&](uint32_t x, uint32_t y) { return keys[x] < keys[y]; });
  for (size_t r = 0; r < LA; ++r) rank[by_rank[r]] = (uint32_t)r;
  // dense matrices over all loci: sum_str_counts (LA x NS) and depth (NS x LA, sample-major for the medians)
  std::vector<double> ssc(LA * NS, NaN), depth(NS * LA, NaN);
  std::vector<int32_t> cell_of(LA * NS, -1);
  parallel_for(NS, T, [&](size_t s) {
    for (size_t j = 0; j < S[s].cells.size(); ++j) {
      const Cell &c = S[s].cells[j];
      const size_t l = rank[c.locus];
      ssc[l * NS + s] = c.ssc;
      depth[s * LA + l] = c.depth;
      cell_of[l * NS + s] = (int32_t)j;
    }
  });
  // :260-262 rows that are all 0 or NaN are dropped
  std::vector<uint8_t> keep(LA, 0);
  std::vector<uint32_t> kept;
  for (size_t l = 0; l < LA; ++l) {
    for (size_t s = 0; s < NS && !keep[l]; ++s) { const double v = ssc[l * NS + s]; keep[l] = !(v != v || v == 0.0); }
    if (keep[l]) kept.push_back((uint32_t)l);
  }
  const size_t L = kept.size();
  if (L == 0 && ctl.loci.empty()) die(1, "ValueError: z score table is empty");
  tm.lap("parse");

  // ---- the device
  strl_ctx *ctx = nullptr;
  CK(strl_ctx_create(0, &ctx));
  tm.lap("device context");
  std::vector<double> m_all(NS), m_kept(NS), m_filled(NS);
  CK(strl_outliers_row_medians(ctx, depth.data(), NS, LA, keep.data(), m_all.data(), m_kept.data(), m_filled.data(), STRL_MEM_HOST));
  tm.lap("depth medians");

  // unplaced.tsv :211-230 (pivot repeatunit x sample, fillna(0), melt; float when the pivot made holes or a count was one)
  {
    std::set<std::string> units;
    bool fl = false;
    size_t cells = 0;
    for (const auto &s : S) { for (const auto &u : s.unplaced) units.insert(u.first); fl |= s.unplaced_float; cells += s.unplaced.size(); }
    fl |= cells < units.size() * NS;
    std::string o = "repeatunit\tsample\tunplaced_count\n";
    for (const auto &s : S) {
      std::map<std::string, double> m(s.unplaced.begin(), s.unplaced.end());
      for (const auto &u : units) {
        const auto it = m.find(u);
        const double v = it == m.end() ? 0.0 : it->second;
        o += u; o += '\t'; o += s.name; o += '\t';
        if (fl) cell_float(v, o); else cell_int((int64_t)v, o);
        o += '\n';
      }
    }
    if (!write_text(a.out + "unplaced.tsv", o)) die(1, "cannot write %sunplaced.tsv", a.out.c_str());
  }
  {   // depths.tsv :247-249
    std::string o = "depth\tsample\n";
    for (size_t s = 0; s < NS; ++s) { cell_float(m_all[s], o); o += '\t'; o += S[s].name; o += '\n'; }
    if (!write_text(a.out + "depths.tsv", o)) die(1, "cannot write %sdepths.tsv", a.out.c_str());
  }

  // ---- sum_str_log :280-290 with the host libm; the null locus :296-300 as one more row
  std::vector<double> X((L + 1) * NS), depf(L * NS);
  parallel_for(L, T, [&](size_t j) {
    const size_t l = kept[j];
    for (size_t s = 0; s < NS; ++s) {
      double d = depth[s * LA + l];
      if (d != d || d == 0.0) d = m_kept[s];
      depf[j * NS + s] = d;
      X[j * NS + s] = log2((ssc[l * NS + s] + 1.0) / d);
    }
  });
  for (size_t s = 0; s < NS; ++s) X[L * NS + s] = log2(1.0 / m_filled[s]);
  tm.lap("sum_str_log");
  double *dX = nullptr;
  CK(strl_dev_alloc(ctx, X.size() * 8, (void **)&dX));
  CK(strl_copy(ctx, dX, X.data(), X.size() * 8, 1));
  tm.lap("upload");
  double *dmu = nullptr, *dsd = nullptr;
  uint8_t *dmeth = nullptr;
  CK(strl_dev_alloc(ctx, (L + 1) * 8, (void **)&dmu));
  CK(strl_dev_alloc(ctx, (L + 1) * 8, (void **)&dsd));
  CK(strl_dev_alloc(ctx, L + 1, (void **)&dmeth));
  CK(strl_outliers_huber(ctx, dX, L + 1, NS, dmu, dsd, dmeth, STRL_MEM_DEVICE));
  std::vector<double> mu(L + 1), sd(L + 1);
  std::vector<uint8_t> meth(L + 1);
  CK(strl_copy(ctx, mu.data(), dmu, (L + 1) * 8, 0));
  CK(strl_copy(ctx, sd.data(), dsd, (L + 1) * 8, 0));
  CK(strl_copy(ctx, meth.data(), dmeth, L + 1, 0));
  tm.lap("huber");

  if (!a.emit.empty()) {          // :329-336 (NaN written as an empty field)
    std::string o = "locus\tmu\tsd\tn\n";
    auto ef = [&](double v) { if (v == v) py_repr(v, o); };
    for (size_t j = 0; j <= L; ++j) {
      if (j < L) o.append(keys[by_rank[kept[j]]]); else o += "null_locus_counts";
      o += '\t'; ef(mu[j]); o += '\t'; ef(sd[j]); o += '\t';
      o += std::to_string(NS);
      o += '\n';
    }
    if (!write_text(a.emit, o)) die(1, "cannot write %s", a.emit.c_str());
  }

  // ---- z / p / p_adj :340-404
  size_t n_null = 0;
  std::vector<double> null_mu, null_sd;
  if (!a.control.empty()) {
    std::vector<double> umu(L), usd(L);
    for (size_t j = 0; j < L; ++j) {
      const auto it = ctl.est.find(std::string(keys[by_rank[kept[j]]]));
      double m = it == ctl.est.end() ? NaN : it->second.first, d = it == ctl.est.end() ? NaN : it->second.second;
      umu[j] = m == m ? m : ctl.null_mu;                    // reindex + fillna with the null row :348-351
      usd[j] = d == d ? d : ctl.null_sd;
    }
    CK(strl_copy(ctx, dmu, umu.data(), L * 8, 1));
    CK(strl_copy(ctx, dsd, usd.data(), L * 8, 1));
    std::unordered_map<std::string_view, bool> have;
    for (size_t j = 0; j < L; ++j) have[keys[by_rank[kept[j]]]] = true;
    for (const auto &l : ctl.loci)
      if (!have.count(l)) {
        null_mu.push_back(ctl.est[l].first);
        null_sd.push_back(ctl.est[l].second);
      }
    n_null = null_mu.size();
  }
  if (L + n_null == 0) die(1, "ValueError: z score table is empty");
  double *dz = nullptr, *dp = nullptr, *dq = nullptr, *dnm = nullptr, *dns = nullptr, *da2 = nullptr;
  const size_t LS = L * NS;
  CK(strl_dev_alloc(ctx, LS * 8, (void **)&dz));
  CK(strl_dev_alloc(ctx, LS * 8, (void **)&dp));
  CK(strl_dev_alloc(ctx, LS * 8, (void **)&dq));
  if (n_null) {
    CK(strl_dev_alloc(ctx, n_null * 8, (void **)&dnm));
    CK(strl_dev_alloc(ctx, n_null * 8, (void **)&dns));
    CK(strl_copy(ctx, dnm, null_mu.data(), n_null * 8, 1));
    CK(strl_copy(ctx, dns, null_sd.data(), n_null * 8, 1));
  }
  // the control-only rows hold NaN (the script's fillna at :368 aligns a sample-indexed frame on the loci axis): null_x = NULL
  CK(strl_outliers_scores(ctx, dX, dmu, dsd, L, NS, nullptr, dnm, dns, n_null, dz, dp, dq, STRL_MEM_DEVICE));
  tm.lap("z / p / BH");

  // ---- order :451
  std::vector<double> a2(LS);
  parallel_for(L, T, [&](size_t j) {
    const size_t l = kept[j];
    for (size_t s = 0; s < NS; ++s) { const int32_t c = cell_of[l * NS + s]; a2[j * NS + s] = c < 0 ? NaN : S[s].cells[(size_t)c].a2; }
  });
  CK(strl_dev_alloc(ctx, LS * 8, (void **)&da2));
  CK(strl_copy(ctx, da2, a2.data(), LS * 8, 1));
  uint32_t *dord = nullptr;
  CK(strl_dev_alloc(ctx, LS * 4 + 4, (void **)&dord));
  CK(strl_outliers_order(ctx, dz, da2, L, NS, dord, STRL_MEM_DEVICE));
  std::vector<uint32_t> order(LS);
  std::vector<double> z(LS), p(LS), q(LS);
  CK(strl_copy(ctx, order.data(), dord, LS * 4, 0));
  CK(strl_copy(ctx, z.data(), dz, LS * 8, 0));
  CK(strl_copy(ctx, p.data(), dp, LS * 8, 0));
  CK(strl_copy(ctx, q.data(), dq, LS * 8, 0));
  for (void *ptr : {(void *)dX, (void *)dmu, (void *)dsd, (void *)dmeth, (void *)dz, (void *)dp, (void *)dq, (void *)dnm, (void *)dns,
                    (void *)da2, (void *)dord})
    CK(strl_dev_free(ctx, ptr));
  tm.lap("order");

  // ---- STRs.tsv and <sample>.STRs.tsv :435-473
  std::string head = "chrom\tleft\tright\tlocus\tsample\trepeatunit\tallele1_est\tallele2_est\tspanning_reads\tspanning_pairs\t"
                     "left_clips\tright_clips\tunplaced_pairs\tsum_str_counts\tsum_str_log\tdepth\toutlier\tp\tp_adj";
  if (a.debug) head += "\tmethod";
  head += '\n';
  const size_t CH = 1 << 16;
  const size_t nch = (LS + CH - 1) / CH;
  std::vector<std::string> text(nch);
  std::vector<std::vector<uint32_t>> row_end(nch);
  std::vector<uint8_t> in_sample(LS);
  parallel_for(nch, T, [&](size_t ci) {
    std::string &o = text[ci];
    std::vector<uint32_t> &ends = row_end[ci];
    for (size_t k = ci * CH; k < std::min(LS, (ci + 1) * CH); ++k) {
      const size_t idx = order[k], j = idx / NS, s = idx % NS, l = kept[j];
      const int32_t ci2 = cell_of[l * NS + s];
      const Cell *c = ci2 < 0 ? nullptr : &S[s].cells[(size_t)ci2];
      const std::string_view key = keys[by_rank[l]];
      if (c) {
        o.append(key.substr(0, c->chrom_len)); o += '\t';
        cell_int(c->left, o); o += '\t'; cell_int(c->right, o); o += '\t';
      } else o += "NaN\t0\t0\t";                                           // fillna(0) :274-275
      o.append(key); o += '\t';
      o += S[s].name; o += '\t';
      if (c) { o.append(key.substr(key.rfind('-') + 1)); o += '\t'; } else o += "NaN\t";
      cell_float(c ? c->a1 : NaN, o); o += '\t';
      cell_float(c ? c->a2 : NaN, o); o += '\t';
      for (int t = 0; t < 5; ++t) { cell_int(c ? c->ints[t] : INT_NA, o); o += '\t'; }
      const double cnt = ssc[l * NS + s];
      cell_int(cnt != cnt ? INT_NA : (int64_t)cnt, o); o += '\t';
      cell_round1(X[j * NS + s], o); o += '\t';
      cell_float(depf[j * NS + s], o); o += '\t';
      cell_g2(z[idx], o); o += '\t';
      cell_g2(p[idx], o); o += '\t';
      cell_g2(q[idx], o);
      if (a.debug) { o += '\t'; o += meth[j] ? "MAD" : "Huber"; }
      o += '\n';
      ends.push_back((uint32_t)o.size());
      // :467-468 the per-sample filters (NaN allele2_est fails any comparison)
      bool ok = c && c->a2 >= (double)a.min_size;
      if (ok) ok = (int64_t)c->ints[2] + c->ints[3] >= a.min_clips;
      in_sample[k] = ok;
    }
  });
  {
    FILE *f = fopen((a.out + "STRs.tsv").c_str(), "wb");
    if (!f) die(1, "cannot write %sSTRs.tsv", a.out.c_str());
    fputs(head.c_str(), f);
    for (const auto &t : text) fwrite(t.data(), 1, t.size(), f);
    if (fclose(f)) die(1, "cannot write %sSTRs.tsv", a.out.c_str());
  }
  std::vector<std::vector<uint32_t>> rows_of(NS);
  for (size_t k = 0; k < LS; ++k)
    if (in_sample[k]) rows_of[order[k] % NS].push_back((uint32_t)k);
  parallel_for(NS, T, [&](size_t s) {
    std::string o = head;
    for (const uint32_t k : rows_of[s]) {
      const size_t ci = k / CH, r = k % CH;
      const uint32_t b = r ? row_end[ci][r - 1] : 0, e = row_end[ci][r];
      o.append(text[ci], b, e - b);
    }
    if (!write_text(a.out + S[s].name + ".STRs.tsv", o)) die(1, "cannot write %s%s.STRs.tsv", a.out.c_str(), S[s].name.c_str());
  });
  tm.lap("format / write");
  strl_ctx_destroy(ctx);
  if (a.verbose) {
    std::string j = "{";
    double tot = 0;
    for (const auto &lp : tm.laps) { char b[96]; snprintf(b, sizeof b, "%s\"%s\": %.4f", j.size() > 1 ? ", " : "", lp.first.c_str(), lp.second); j += b; tot += lp.second; }
    char b[64];
    snprintf(b, sizeof b, ", \"total\": %.4f}", tot);
    j += b;
    fprintf(stderr, "[strling outliers] samples %zu loci %zu (kept %zu) cells %zu seconds %s\n", NS, LA, L, LS, j.c_str());
  }
  return 0;
}
