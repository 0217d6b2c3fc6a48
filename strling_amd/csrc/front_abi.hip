// front_abi.hip -- the C-ABI entry points of the device BAM front end (strl_front_*): they drive the kernels of front.hip chunk
// by chunk and hand every parsed chunk to the chunked extract (extract.hip).
#include <string.h>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <memory>
#include <string>
#include <thread>
#include <vector>
#include "common.h"
#include "front.h"
#include "sort.h"

using namespace strl;

extern "C" {

// ---- `strling extract` with the BAM front end on the device (front.hip): the host hands over BGZF blocks, never a record ----
static int front_fill_done(strl_ctx *c, strl::FrontSlot &S, strl_front_chunk *done) {
  STRL_HIP(hipEventSynchronize(S.ev_b));
  S.b_pending = false;
  const strl::FrontInfo &I = S.h_info[1];
  if (I.err & strl::FRONT_ERR_LSEQ) { set_error("a record's l_seq is outside [0, %d]", STRL_MAX_READ_LEN); return STRL_ERR_ARG; }   // (kept: stage B refuses the chunk before the parse)
  if (done) {
    done->n_records = I.n_records; done->n_primary = I.n_primary; done->last_placed = I.last_placed; done->tail_primary = I.tail_primary;
    done->max_l_seq = I.max_l_seq; done->scan_slow_segments = I.slow_segments;
  }
  return STRL_OK;
}

// the full-size per-read buffers are there (or the small ones are full: then this waits for them): what the chunks so far have
// filled is copied over on the context's stream -- behind every kernel that wrote it -- and the small buffers are kept until the
// front end goes (nothing waits for them to be free)
static int front_adopt_big(strl_ctx *c, strl::strl_front *F, uint64_t at) {
  std::unique_ptr<strl::FrontBigAlloc> B(F->big);      // (whatever the front end does not adopt goes with it, on every return)
  if (!B) return STRL_OK;
  if (B->th.joinable()) B->th.join();
  F->big = nullptr;
  if (B->rc) { set_error("%s", B->err.c_str()); return B->rc; }
  struct Mv { strl::DevBuf *cur, *big; size_t used; };
  const Mv mv[6] = {{&c->x_rows, &B->rows, (size_t)at * sizeof(strl_pair_rec)}, {&c->x_qhash, &B->qhash, (size_t)at * 8}, {&c->x_whole, &B->whole, (size_t)at * 4},
                    {&F->qref, &B->qref, (size_t)at * 8}, {&F->fragw, &B->fragw, (size_t)at * 4}, {&F->qarena, &B->qarena, (size_t)F->qarena_used}};
  for (const Mv &m : mv) {
    if (m.big->cap <= m.cur->cap) { m.big->release(); continue; }        // (the small one grew past it meanwhile)
    if (m.used) STRL_HIP(hipMemcpyAsync(m.big->p, m.cur->p, std::min(m.used, m.cur->cap), hipMemcpyDeviceToDevice, c->stream));
    F->trash.push_back(std::move(*m.cur));
    *m.cur = std::move(*m.big);
  }
  return STRL_OK;
}

// parse + score the chunk in slot si (its record scan was enqueued earlier): waits on the HOST for the scan's counts -- the
// next chunk's inflate is already queued behind it, so the device does not idle
static int front_stage_b(strl_ctx *c, strl::strl_front *F, int si) {
  using namespace strl;
  FrontSlot &S = F->slot[si];
  STRL_HIP(hipEventSynchronize(S.ev_a));
  const FrontInfo I = S.h_info[0];
  if (I.err & FRONT_ERR_INFLATE) { set_error("invalid BGZF block (DEFLATE data or ISIZE)"); return STRL_ERR_FORMAT; }
  if (I.err & FRONT_ERR_CRC) { set_error("CRC32 checksum mismatch in a BGZF block"); return STRL_ERR_CRC; }
  if (I.err & FRONT_ERR_RECORD) { set_error("malformed BAM record"); return STRL_ERR_FORMAT; }
  if (I.err & FRONT_ERR_CARRY) { set_error("BAM record of more than %u bytes", FRONT_CARRY_MAX); return STRL_ERR_FORMAT; }
  const uint64_t n = I.n_records, at = c->x_n;
  if (at + n > strl_record_limit()) { set_error("chunked extract: more than %llu records in one device pass", (unsigned long long)strl_record_limit()); return STRL_ERR_LIMIT; }
  if (I.max_l_seq > (uint32_t)STRL_MAX_READ_LEN) { set_error("a record's l_seq %u is outside [0, %d]", I.max_l_seq, STRL_MAX_READ_LEN); return STRL_ERR_ARG; }
  int rc;       // (records of STRL_DEVICE_READ_LEN < l_seq <= STRL_MAX_READ_LEN bases: scored by the host twin inside score_device)
  const uint64_t n1 = std::max<uint64_t>(n, 1);
  if (F->big && (F->big->done.load(std::memory_order_acquire) || at + n1 > F->small_reads || F->qarena_used + I.qname_bytes + 16 > F->qarena.cap) && (rc = front_adopt_big(c, F, at))) return rc;
  if ((rc = c->x_rows.grow((size_t)(at + n1) * sizeof(strl_pair_rec), (size_t)at * sizeof(strl_pair_rec), c->stream)) ||
      (rc = c->x_qhash.grow((size_t)(at + n1) * 8, (size_t)at * 8, c->stream)) || (rc = c->x_whole.grow((size_t)(at + n1) * 4, (size_t)at * 4, c->stream)) ||
      (rc = F->qref.grow((size_t)(at + n1) * 8, (size_t)at * 8, c->stream)) || (rc = F->fragw.grow((size_t)(at + n1) * 4, (size_t)at * 4, c->stream)) ||
      (rc = F->qarena.grow((size_t)(F->qarena_used + I.qname_bytes + 16), (size_t)F->qarena_used, c->stream)))
    return rc;
  const uint64_t seq_bytes = I.seq_bytes + 64;
  auto room = [](uint64_t need) { return (size_t)(need + need / 4 + 4096); };
  if (F->s_tid.cap < n1 * 4 && ((rc = F->s_tid.reserve(room(n1 * 4))) || (rc = F->s_pos.reserve(room(n1 * 4))) || (rc = F->s_end.reserve(room(n1 * 4))) ||
                                (rc = F->s_seqoff.reserve(room(n1 * 4))) || (rc = F->s_lseq.reserve(room(n1 * 2))) || (rc = F->s_clipl.reserve(room(n1 * 2))) ||
                                (rc = F->s_clipr.reserve(room(n1 * 2))) || (rc = F->s_mapq.reserve(room(n1))) || (rc = F->s_cig.reserve(room(n1))) ||
                                (rc = F->tidflag.reserve(room(n1))) || (rc = F->s_meta.reserve(room(n1 * 16)))))
    return rc;
  if (F->s_seq4.cap < seq_bytes && (rc = F->s_seq4.reserve(room(seq_bytes)))) return rc;
  FrontParseOut o;
  o.tid = F->s_tid.as<int32_t>(); o.pos = F->s_pos.as<int32_t>(); o.end = F->s_end.as<int32_t>(); o.seq_off = F->s_seqoff.as<uint32_t>();
  o.l_seq = F->s_lseq.as<uint16_t>(); o.clip_l = F->s_clipl.as<uint16_t>(); o.clip_r = F->s_clipr.as<uint16_t>();
  o.mapq = F->s_mapq.as<uint8_t>(); o.cig = F->s_cig.as<uint8_t>(); o.seq4 = F->s_seq4.as<uint8_t>(); o.meta = F->s_meta.as<uint4>();
  o.rows = c->x_rows.as<strl_pair_rec>() + at; o.qhash = c->x_qhash.as<uint64_t>() + at; o.qref = F->qref.as<uint64_t>() + at;
  o.qarena = F->qarena.as<uint8_t>(); o.qarena_at = F->qarena_used; o.fragw = F->fragw.as<uint32_t>() + at; o.tidflag = F->tidflag.as<uint8_t>();
  // (the scan finished: the host waited for it.  The previous chunk's scorer may still read the chunk-temporary columns:
  // same stream, so the parse queues behind it.)
  if ((rc = front_parse(c, F, si, (uint32_t)n, o, c->stream))) return rc;
  F->qarena_used += I.qname_bytes;
  if (c->bai) bai_front_index(c, F, si, I, o.tid, o.pos, o.end, o.fragw);       // extract --write-index: the columns just written are its input
  if (n) {
    strl_read_soa d{};
    d.n = n; d.tid = o.tid; d.pos = o.pos; d.end = o.end; d.seq_off = o.seq_off; d.l_seq = o.l_seq; d.clip_l = o.clip_l; d.clip_r = o.clip_r;
    d.mapq = o.mapq; d.cig = o.cig; d.seq4 = o.seq4; d.seq4_bytes = seq_bytes; d.max_l_seq = I.max_l_seq; d.mem = STRL_MEM_DEVICE;
    d.meta = reinterpret_cast<const strl_read_meta *>(o.meta);
    if ((rc = extract_add_scored(c, &d, at))) return rc;
  }
  STRL_HIP(hipEventRecord(S.ev_b, c->stream));
  S.b_pending = true;
  return STRL_OK;
}

int strl_front_begin(strl_ctx *c, int32_t n_ref, uint64_t first_record_offset, uint64_t n_reads_hint) {
  if (!c || n_ref < 0) { set_error("bad argument"); return STRL_ERR_ARG; }
  const uint64_t hint = std::max<uint64_t>(n_reads_hint, 1 << 20);
  // (STRL_ASYNC_ALLOC=1: the full-size buffers on a thread beside the first chunks, front.h.  Measured: 0.15 -> 0.03 s in front of
  // the loop at 1.3e8 reads, but the loop pays for it -- at 5.4e8 reads 2.60 s against 2.41 s with everything allocated up
  // front, wall 2.99 against 2.80 s (profiles/r05/full_size_shares.log): allocating tens of gigabytes beside running kernels
  // slows the launches down by more than it hides.  Off by default.)
  static const bool sync_alloc = getenv("STRL_ASYNC_ALLOC") == nullptr;
  const uint64_t small = (sync_alloc || hint <= (1ull << 25)) ? hint : std::max<uint64_t>(1ull << 24, hint / 8);
  // The per-read state of a whole file is tens of gigabytes in seven buffers.  hipMalloc returns at once for them on a settled
  // device (0.03 s for all of a whole genome's), but a large allocation made while the driver still reclaims what an earlier
  // process held stalls for ~0.48 s -- each one (profiles/r06/state_alloc_diag.log: 23 GB 0.483 s, 17.5 GB 0.483 s, 5.9 GB 0.121 s
  // in the first process on a box, one 0.483 s in the second, none from the third on).  Made side by side, the stalls overlap.
  STRL_HIP(hipSetDevice(c->device));
  STRL_HIP(hipStreamSynchronize(c->stream));
  strl::DevBuf pre_qref, pre_fragw, pre_qarena;
  // ... and the front end's four streams beside them: a stream is ~9.5 ms of the runtime's time here (profiles/r06/ctx_laps.log),
  // made one after the other behind the allocations they were most of this call
  hipStream_t pre_st[4] = {nullptr, nullptr, nullptr, nullptr};       // inflate 0, inflate 1, record scan, copies
  int pre_st_rc[4] = {0, 0, 0, 0};
  {
    struct Want { strl::DevBuf *b; size_t bytes; int rc; std::string err; };
    // ... and with them what the pair pass over the whole file takes at the END (strl_extract_finish -> strl_pair_device: join items,
    // emission keys, treads, the sort's scratch -- 4 GB for a genome).  Allocated there, behind the loop, they made that pass 0.05 -
    // 0.09 s in this round's earlier lines (0.016 s in round 5's); in place beforehand it is 0.016 - 0.017 s in six runs of six
    // (profiles/r06/pair_prealloc_full_size.log).  Sized as that call sizes them for `hint` reads, so that it finds them in place
    const uint64_t p_icap = std::max<uint64_t>(std::min<uint64_t>(hint / 8 + 65536, 3 * hint + 16), 1024), p_ecap = std::max<uint64_t>(std::min<uint64_t>(hint / 16 + 65536, 8 * hint + 16), 1024);
    int p_ebits = 3;
    while (p_ebits < 40 && ((2 * hint) >> (p_ebits - 2))) ++p_ebits;
    const size_t p_sb = std::max(radix_sort_scratch_bytes((uint32_t)p_icap, 32), radix_sort_scratch_bytes((uint32_t)p_ecap, p_ebits));
    const size_t p_max = (size_t)std::max(p_icap, p_ecap);
    Want want[] = {{&c->x_rows, (size_t)small * sizeof(strl_pair_rec), 0, {}}, {&pre_qarena, (size_t)small * 24, 0, {}}, {&c->x_qhash, (size_t)small * 8, 0, {}},
                   {&pre_qref, (size_t)small * 8, 0, {}}, {&c->x_whole, (size_t)small * 4, 0, {}}, {&pre_fragw, (size_t)small * 4, 0, {}},
                   {&c->x_soft, (size_t)(hint / 8 + 65536) * sizeof(strl_soft_rec), 0, {}},
                   {&c->p_key0, p_max * 8, 0, {}}, {&c->p_key1, p_max * 8, 0, {}}, {&c->p_val0, p_max * 4, 0, {}}, {&c->p_val1, p_max * 4, 0, {}},
                   {&c->p_emit, (size_t)p_ecap * sizeof(strl_tread), 0, {}}, {&c->treads, (size_t)p_ecap * sizeof(strl_tread) + 64, 0, {}}, {&c->sort_scratch, p_sb, 0, {}}};
    const int dev = c->device;
    int least = 0, greatest = 0;          // (numerically: least >= greatest; equal where the device has one level)
    STRL_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest));      // (in front of the threads: nothing may return between their start and their join)
    std::vector<std::thread> th;
    for (Want &w : want)
      th.emplace_back([&w, dev] {
        if (hipSetDevice(dev) != hipSuccess) { w.rc = STRL_ERR_HIP; w.err = "hipSetDevice"; return; }
        if (w.b->cap >= w.bytes && w.b->p) return;
        w.rc = w.b->reserve(w.bytes);
        if (w.rc) w.err = strl_last_error();
      });
    for (int k = 0; k < 4; ++k)
      th.emplace_back([&pre_st, &pre_st_rc, k, dev, least, greatest] {
        hipError_t e = hipSetDevice(dev);
        if (e == hipSuccess) e = k == 3 ? hipStreamCreateWithFlags(&pre_st[k], hipStreamNonBlocking) : hipStreamCreateWithPriority(&pre_st[k], hipStreamNonBlocking, k == 2 ? greatest : least);
        pre_st_rc[k] = (int)e;
      });
    for (auto &t : th) t.join();
    auto drop_streams = [&] { for (hipStream_t &q : pre_st) if (q) { (void)hipStreamDestroy(q); q = nullptr; } };
    for (int k = 0; k < 4; ++k)
      if (pre_st_rc[k]) {
        set_error("hipStreamCreate: %s", hipGetErrorString((hipError_t)pre_st_rc[k]));
        drop_streams();
        return STRL_ERR_HIP;
      }
    for (Want &w : want)
      if (w.rc) {
        set_error("%s", w.err.c_str());
        drop_streams();
        return w.rc;
      }
  }
  int rc = extract_begin_sized(c, n_reads_hint, small);
  if (rc) { for (hipStream_t q : pre_st) if (q) (void)hipStreamDestroy(q); return rc; }
  if (c->front) {
    for (hipStream_t q : c->front->st_i) if (q) (void)hipStreamSynchronize(q);
    if (c->front->st_a) (void)hipStreamSynchronize(c->front->st_a);
    strl::front_destroy(c->front); c->front = nullptr;
  }
  if (c->bai) { strl::bai_destroy(c->bai); c->bai = nullptr; }       // (a builder of the previous pass: everything it had in flight has completed)
  strl::strl_front *F = new strl::strl_front();
  c->front = F;
  c->x_front = true;
  F->qref = std::move(pre_qref); F->fragw = std::move(pre_fragw); F->qarena = std::move(pre_qarena);        // (allocated above, beside the others; the context owns them from here)
  F->n_ref = n_ref; F->first_off = first_record_offset;
  F->st_i[0] = pre_st[0]; F->st_i[1] = pre_st[1]; F->st_a = pre_st[2]; F->st_c = pre_st[3];   // (made above, beside the allocations)
  if ((rc = strl::front_init_slots(c, F))) return rc;
  if ((rc = F->tid_seen.reserve((size_t)n_ref + 16))) return rc;
  STRL_HIP(hipMemsetAsync(F->tid_seen.p, 0, (size_t)n_ref + 16, c->stream));
  if ((rc = F->qref.grow((size_t)small * 8, 0, c->stream)) || (rc = F->fragw.grow((size_t)small * 4, 0, c->stream)) || (rc = F->qarena.grow((size_t)small * 24, 0, c->stream)))
    return rc;
  F->small_reads = small;
  if (small < hint) {        // the full-size buffers: allocated beside the first chunks (front.h, FrontBigAlloc)
    strl::FrontBigAlloc *B = new strl::FrontBigAlloc();
    F->big = B;
    const int dev = c->device;
    B->th = std::thread([B, dev, hint] {
      auto one = [&](strl::DevBuf &b, size_t bytes) {
        if (hipSetDevice(dev) != hipSuccess) return (int)STRL_ERR_HIP;
        return b.reserve(bytes);
      };
      // (side by side: the driver takes several allocations at once)
      int r[6] = {0, 0, 0, 0, 0, 0};
      std::thread t1([&] { r[0] = one(B->rows, (size_t)hint * sizeof(strl_pair_rec)); });
      std::thread t2([&] { r[1] = one(B->qarena, (size_t)hint * 24); });
      std::thread t3([&] { r[2] = one(B->qhash, (size_t)hint * 8); r[3] = one(B->qref, (size_t)hint * 8); });
      r[4] = one(B->whole, (size_t)hint * 4); r[5] = one(B->fragw, (size_t)hint * 4);
      t1.join(); t2.join(); t3.join();
      for (int x : r) if (x && !B->rc) { B->rc = x; B->err = strl_last_error(); }
      B->done.store(1, std::memory_order_release);
    });
  }
  STRL_HIP(hipStreamSynchronize(c->stream));
  return STRL_OK;
}

int strl_front_push(strl_ctx *c, const uint8_t *comp, uint64_t comp_bytes, const uint64_t *coff, const uint32_t *clen, const uint32_t *isize, const uint32_t *crc32,
                    uint32_t n_blocks, strl_front_chunk *done, int *n_done) {
  return strl_front_push_after(c, nullptr, comp, comp_bytes, coff, clen, isize, crc32, n_blocks, done, n_done);
}

// the same when the chunks of ONE file go round-robin over several contexts (`strling extract --gpus N`): `prev` = the
// context the previous chunk of the file was pushed to (null / c itself: this context) -- the partial record in front of
// this chunk is taken from there
int strl_front_push_after(strl_ctx *c, strl_ctx *prev, const uint8_t *comp, uint64_t comp_bytes, const uint64_t *coff, const uint32_t *clen, const uint32_t *isize,
                          const uint32_t *crc32, uint32_t n_blocks, strl_front_chunk *done, int *n_done) {
  const int rc = strl_front_enqueue_after(c, prev, comp, comp_bytes, coff, clen, isize, crc32, n_blocks, done, n_done);
  return rc ? rc : strl_front_collect(c);
}

// the two halves of a push, for a caller that has something to do between them (strl_front_stage of the chunk after this
// one): enqueue = this chunk's copy (unless staged) + inflate + record scan, and the summary of the chunk two back;
// collect = wait for the PREVIOUS chunk's record scan, enqueue its parse + scoring
int strl_front_collect(strl_ctx *c) {
  if (!c || !c->front) { set_error("strl_front_collect without strl_front_begin"); return STRL_ERR_ARG; }
  STRL_HIP(hipSetDevice(c->device));
  strl::strl_front *F = c->front;
  int rc;
  while (F->b_issued + 1 < F->chunks) {
    if ((rc = front_stage_b(c, F, (int)(F->b_issued & 1)))) return rc;
    ++F->b_issued;
  }
  return STRL_OK;
}

int strl_front_trim_next(strl_ctx *c, uint32_t tail_bytes) {
  if (!c || !c->front || !c->x_open) { set_error("strl_front_trim_next without strl_front_begin"); return STRL_ERR_ARG; }
  if (tail_bytes > 65536u) { set_error("strl_front_trim_next: more than a BGZF block"); return STRL_ERR_ARG; }
  c->front->next_trim = tail_bytes;
  return STRL_OK;
}

// bytes behind the last complete record of the last chunk handed over (after strl_front_finish: every scan has been waited for)
int strl_front_tail_bytes(strl_ctx *c, uint32_t *tail_bytes) {
  if (!c || !c->front || !tail_bytes) { set_error("strl_front_tail_bytes: bad argument"); return STRL_ERR_ARG; }
  strl::strl_front *F = c->front;
  if (F->b_issued < F->chunks) { set_error("strl_front_tail_bytes before strl_front_finish"); return STRL_ERR_ARG; }
  *tail_bytes = F->last_slot < 0 ? 0u : F->slot[F->last_slot].h_info[0].carry_len;
  return STRL_OK;
}

int strl_front_reserve(strl_ctx *c, uint32_t max_blocks, uint64_t max_comp_bytes) {
  if (!c || !c->front || !max_blocks) { set_error("strl_front_reserve: bad argument / no strl_front_begin"); return STRL_ERR_ARG; }
  STRL_HIP(hipSetDevice(c->device));
  // (the parse columns and the scorer's per-chunk queues are left to their first full chunk: reserving them here too cost
  // 40 - 60 ms of hipMalloc before the loop against 8 ms of one late inflate inside it)
  return strl::front_reserve(c, c->front, max_blocks, max_comp_bytes);
}

// starts the copy to the device of the chunk the NEXT strl_front_push / _enqueue_after of this context will hand over -- or, if that
// one is staged already, of the chunk after it
int strl_front_stage(strl_ctx *c, const uint8_t *comp, uint64_t comp_bytes, const uint64_t *coff, const uint32_t *clen, const uint32_t *isize, const uint32_t *crc32,
                     uint32_t n_blocks) {
  if (!c || !c->front || !c->x_open || !n_blocks || !comp || !coff || !clen || !isize) { set_error("strl_front_stage: bad argument / no strl_front_begin"); return STRL_ERR_ARG; }
  STRL_HIP(hipSetDevice(c->device));
  strl::strl_front *F = c->front;
  int si = (int)(F->chunks & 1);
  if (F->slot[si].staged) si ^= 1;          // the next push's chunk is staged: this is the one behind it (the caller stages in file order)
  if (F->slot[si].staged) { set_error("strl_front_stage: two chunks are staged already"); return STRL_ERR_ARG; }
  const strl::FrontChunkDesc d{comp, comp_bytes, coff, clen, isize, crc32, n_blocks};
  return strl::front_copy(c, F, si, d);
}

int strl_front_enqueue_after(strl_ctx *c, strl_ctx *prev, const uint8_t *comp, uint64_t comp_bytes, const uint64_t *coff, const uint32_t *clen, const uint32_t *isize,
                             const uint32_t *crc32, uint32_t n_blocks, strl_front_chunk *done, int *n_done) {
  if (!c || !c->front || !c->x_open || (n_blocks && (!comp || !coff || !clen || !isize))) { set_error("strl_front_push: bad argument / no strl_front_begin"); return STRL_ERR_ARG; }
  if (prev == c) prev = nullptr;
  if (prev && (!prev->front || prev->front->last_slot < 0)) { set_error("strl_front_push_after: the previous context has no chunk"); return STRL_ERR_ARG; }
  STRL_HIP(hipSetDevice(c->device));
  strl::strl_front *F = c->front;
  if (n_done) *n_done = 0;
  if (!n_blocks) return STRL_OK;
  const int si = (int)(F->chunks & 1);
  int rc;
  if ((rc = strl_front_collect(c))) return rc;        // (a caller that left it out: the slot's previous occupant must have been handed to the scorer)
  const bool reuse = F->slot[si].b_pending;          // the chunk before the previous one: its slot is reused now
  const strl::FrontChunkDesc d{comp, comp_bytes, coff, clen, isize, crc32, n_blocks};
  if (prev) {
    strl::FrontSlot &PS = prev->front->slot[prev->front->last_slot];
    const strl::FrontCarrySrc cs{PS.infl.as<uint8_t>(), PS.info.as<strl::FrontInfo>(), prev->front->last_end, prev->device, PS.ev_a, &PS.wait_read, &PS.read_pending};
    rc = strl::front_stage_a(c, F, si, d, false, &cs);
  } else {
    rc = strl::front_stage_a(c, F, si, d, F->chunks == 0 && !F->not_first);
  }
  if (rc) return rc;
  // The summary of the slot's previous occupant is waited for AFTER this chunk's work has been queued (the device waits for
  // that parse itself, ev_b).  The other order kept this chunk's copy to the device from being queued until the parse two
  // chunks back had finished -- it runs beside an inflate that leaves it few wave slots, up to 16 ms -- and every second
  // inflate started 7 ms late (profiles/r04/extract_timeline_before.txt).
  if (reuse) {
    if ((rc = front_fill_done(c, F->slot[si], done))) return rc;
    if (n_done) *n_done = 1;
  }
  if (c->bai) strl::bai_front_chunk(c, si, isize, n_blocks, !prev && !F->not_first && !F->slot[si].staged_trim);
  ++F->chunks;
  F->comp_total += comp_bytes;
  F->infl_total += F->slot[si].infl_bytes;
  return STRL_OK;
}

int strl_front_finish(strl_ctx *c, strl_front_chunk done[2], int *n_done) {
  if (!c || !c->front) { set_error("strl_front_finish without strl_front_begin"); return STRL_ERR_ARG; }
  STRL_HIP(hipSetDevice(c->device));
  strl::strl_front *F = c->front;
  if (n_done) *n_done = 0;
  int rc, k = 0;
  if (!F->chunks) return STRL_OK;
  const int last = (int)((F->chunks - 1) & 1);
  for (; F->b_issued < F->chunks; ++F->b_issued)
    if ((rc = front_stage_b(c, F, (int)(F->b_issued & 1)))) return rc;
  if (F->big && (rc = front_adopt_big(c, F, c->x_n))) return rc;        // (a file shorter than its hint: the thread is joined here at the latest)
  for (int si : {last ^ 1, last}) {
    if (!F->slot[si].b_pending) continue;
    if ((rc = front_fill_done(c, F->slot[si], done ? &done[k] : nullptr))) return rc;
    ++k;
  }
  if (n_done) *n_done = k;
  static const bool timing = getenv("STRL_FRONT_TIMING") != nullptr;
  if (timing && F->tev.size() >= 5) {       // per chunk: [0] start [1] copies queued [2] inflate done [3] ... scan done
    STRL_HIP(hipStreamSynchronize(F->st_a));
    for (hipStream_t q : F->st_i) STRL_HIP(hipStreamSynchronize(q));
    // inflate: the time at least one chunk's inflate was running (consecutive chunks' launches overlap); the other two: sums
    double h2d = 0, inf = 0, scan = 0, open_until = 0;
    for (size_t i = 0; i + 3 < F->tev.size(); i += 4) {
      float a = 0, b0 = 0, b1 = 0, d = 0;
      (void)hipEventElapsedTime(&a, F->tev[i], F->tev[i + 1]);
      (void)hipEventElapsedTime(&b0, F->tev[1], F->tev[i + 1]);
      (void)hipEventElapsedTime(&b1, F->tev[1], F->tev[i + 2]);
      (void)hipEventElapsedTime(&d, F->tev[i + 2], F->tev[i + 3]);
      h2d += a; scan += d;
      const double lo = std::max<double>(b0, open_until);
      if (b1 > lo) { inf += b1 - lo; open_until = b1; }
    }
    fprintf(stderr, "[strling] device front end, ms over %llu chunks: copies to the device %.1f  inflate %.1f  record scan %.1f  (%.1f MB compressed -> %.1f MB inflated)\n",
            (unsigned long long)F->chunks, h2d, inf, scan, (double)F->comp_total / 1e6, (double)F->infl_total / 1e6);
  }
  return STRL_OK;
}

int strl_front_fragwords(strl_ctx *c, uint64_t first, uint64_t n, uint32_t *out) {
  if (!c || !c->front || (n && !out) || first + n > c->x_n) { set_error("strl_front_fragwords: bad range"); return STRL_ERR_ARG; }
  STRL_HIP(hipSetDevice(c->device));
  if (n) STRL_HIP(hipMemcpyAsync(out, c->front->fragw.as<uint32_t>() + first, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
  STRL_HIP(hipStreamSynchronize(c->stream));
  return STRL_OK;
}

// the same without waiting: the copy is enqueued behind the parse of every chunk handed over so far (`out` page-locked);
// *done receives an event for strl_event_wait -- from any thread, so the fragment-length histogram of the first two million
// records can be made beside the rest of the file
int strl_front_fragwords_async(strl_ctx *c, uint64_t first, uint64_t n, uint32_t *out, void **done) {
  if (!c || !c->front || !done || (n && !out) || first + n > c->x_n) { set_error("strl_front_fragwords_async: bad range"); return STRL_ERR_ARG; }
  STRL_HIP(hipSetDevice(c->device));
  hipEvent_t ev;
  STRL_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  if (n) STRL_HIP(hipMemcpyAsync(out, c->front->fragw.as<uint32_t>() + first, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
  STRL_HIP(hipEventRecord(ev, c->stream));
  *done = ev;
  return STRL_OK;
}
// the extraction the front end fed is given up (the context stays; the buffers stay allocated until the context goes or the next
// strl_front_begin): a caller that used the front end for a PREFIX of a file -- `strling call`'s fragment-length sample,
// call.nim:92 -- and goes on to other work on the context.  Everything the front end had in flight has completed on return.
int strl_front_end(strl_ctx *c) {
  if (!c) { set_error("null argument"); return STRL_ERR_ARG; }
  STRL_HIP(hipSetDevice(c->device));
  if (c->front) {
    for (hipStream_t q : c->front->st_i) if (q) (void)hipStreamSynchronize(q);
    if (c->front->st_a) (void)hipStreamSynchronize(c->front->st_a);
    if (c->front->st_c) (void)hipStreamSynchronize(c->front->st_c);
  }
  STRL_HIP(hipStreamSynchronize(c->stream));
  { const int rcj = side_join(c); if (rcj) return rcj; }
  // (nothing is freed here: every hipFree synchronises the device -- 24 ms for the front end's twenty-odd buffers, in front of the
  // caller's next phase.  The buffers go with the context, or with the next strl_front_begin.)
  c->x_open = false; c->x_mode = false; c->x_n = 0;
  return STRL_OK;
}

int strl_front_records(strl_ctx *c, uint64_t *n) {
  if (!c || !n) { set_error("null argument"); return STRL_ERR_ARG; }
  *n = c->x_n;
  return STRL_OK;
}

int strl_front_tids(strl_ctx *c, uint8_t *seen, int32_t n_ref) {
  if (!c || !c->front || n_ref > c->front->n_ref || (n_ref && !seen)) { set_error("strl_front_tids: bad argument"); return STRL_ERR_ARG; }
  STRL_HIP(hipSetDevice(c->device));
  if (n_ref) STRL_HIP(hipMemcpyAsync(seen, c->front->tid_seen.p, (size_t)n_ref, hipMemcpyDeviceToHost, c->stream));
  STRL_HIP(hipStreamSynchronize(c->stream));
  return STRL_OK;
}

int strl_front_qnames(strl_ctx *c, const int64_t *record_ids, uint64_t n, uint64_t *qname_off, char *names, uint64_t cap, uint64_t *need) {
  if (!c || !c->front || (n && (!record_ids || !qname_off))) { set_error("strl_front_qnames: bad argument"); return STRL_ERR_ARG; }
  STRL_HIP(hipSetDevice(c->device));
  strl::strl_front *F = c->front;
  if (qname_off) qname_off[0] = 0;
  if (need) *need = 0;
  if (!n) return STRL_OK;
  if (n > 0x7fffffffull) { set_error("strl_front_qnames: too many names"); return STRL_ERR_ARG; }
  std::vector<uint32_t> ids((size_t)n);
  for (uint64_t i = 0; i < n; ++i) {
    if (record_ids[i] < 0 || (uint64_t)record_ids[i] >= c->x_n) { set_error("strl_front_qnames: record %lld out of range", (long long)record_ids[i]); return STRL_ERR_ARG; }
    ids[(size_t)i] = (uint32_t)record_ids[i];
  }
  strl::DevBuf d_ids, d_ref, d_off, d_out;
  int rc;
  if ((rc = d_ids.reserve((size_t)n * 4)) || (rc = d_ref.reserve((size_t)n * 8)) || (rc = d_off.reserve((size_t)n * 8))) return rc;
  STRL_HIP(hipMemcpyAsync(d_ids.p, ids.data(), (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
  if ((rc = strl::front_gather_names(c, F, d_ids.as<uint32_t>(), (uint32_t)n, d_ref.as<uint64_t>(), c->stream))) return rc;
  std::vector<uint64_t> ref((size_t)n);
  STRL_HIP(hipMemcpyAsync(ref.data(), d_ref.p, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
  STRL_HIP(hipStreamSynchronize(c->stream));
  uint64_t tot = 0;
  for (uint64_t i = 0; i < n; ++i) { qname_off[i] = tot; tot += ref[(size_t)i] & 255u; }
  qname_off[n] = tot;
  if (need) *need = tot;
  if (tot > cap || (tot && !names)) { set_error("strl_front_qnames: %llu bytes of names, capacity %llu", (unsigned long long)tot, (unsigned long long)cap); return STRL_ERR_CAPACITY; }
  if (tot) {
    if ((rc = d_out.reserve((size_t)tot))) return rc;
    STRL_HIP(hipMemcpyAsync(d_off.p, qname_off, (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
    if ((rc = strl::front_copy_names(c, F, d_ref.as<uint64_t>(), d_off.as<uint64_t>(), (uint32_t)n, d_out.as<uint8_t>(), c->stream))) return rc;
    STRL_HIP(hipMemcpyAsync(names, d_out.p, (size_t)tot, hipMemcpyDeviceToHost, c->stream));
    STRL_HIP(hipStreamSynchronize(c->stream));
  }
  return STRL_OK;
}

// Treads of the last extract in .bin order WITH their qnames, in one go: strl_treads_fetch + strl_front_qnames without the
// host round trips in between (references, exclusive scan of the lengths and byte copies are kernels behind the order sort).
// treads[cap] / qname_off[cap + 1] / names[names_cap] may be page-locked memory (then the copies need no staging).
// tread.qname_id stays the record index.  STRL_ERR_CAPACITY with *n_out / *names_need set when something does not fit.
int strl_front_treads_named(strl_ctx *c, strl_tread *treads, uint64_t cap, uint64_t *n_out, uint64_t *qname_off, char *names, uint64_t names_cap, uint64_t *names_need) {
  if (!c || !c->front || !n_out) { set_error("strl_front_treads_named: bad argument"); return STRL_ERR_ARG; }
  uint64_t nt = 0;
  int rc = strl_treads_fetch(c, nullptr, 0, &nt, nullptr);       // orders the treads, checks the error flags
  *n_out = nt;
  if (rc) return rc;
  if (names_need) *names_need = 0;
  if (!treads) return STRL_OK;
  if (nt > cap) { set_error("tread capacity %llu too small, need %llu", (unsigned long long)cap, (unsigned long long)nt); return STRL_ERR_CAPACITY; }
  if (qname_off) qname_off[0] = 0;
  if (!nt) return STRL_OK;
  STRL_HIP(hipSetDevice(c->device));
  // Work space: the pair pass's own scratch.  Once the treads are ordered (strl_treads_fetch above, on this stream) the join /
  // emission keys and values, and the unordered treads, are dead until the next pair pass rewrites them -- and an allocation of
  // its own is four hipMalloc + four hipFree, each of which waits for the device.  A buffer of its own only for what does not fit.
  strl::DevBuf own[5];
  const uint64_t ocap = std::max<uint64_t>(std::min<uint64_t>(names_cap, nt * 255), 16);
  auto room = [&](strl::DevBuf &scratch, strl::DevBuf &mine, size_t bytes, void **p) -> int {
    if (scratch.p && scratch.cap >= bytes) { *p = scratch.p; return STRL_OK; }
    const int r = mine.reserve(bytes);
    *p = mine.p;
    return r;
  };
  void *p_ref = nullptr, *p_len = nullptr, *p_off = nullptr, *p_out = nullptr, *p_tiles = nullptr;
  if ((rc = room(c->p_key0, own[0], (size_t)nt * 8, &p_ref)) || (rc = room(c->p_val0, own[1], (size_t)nt * 4, &p_len)) ||
      (rc = room(c->p_key1, own[2], (size_t)(nt + 1) * 8, &p_off)) || (rc = room(c->p_emit, own[3], (size_t)ocap, &p_out)) ||
      (rc = room(c->p_val1, own[4], strl::front_name_tiles((uint32_t)nt) * 8, &p_tiles)))
    return rc;
  hipStream_t st = c->stream;
  static const bool lap_on = getenv("STRL_FRONT_TIMING") != nullptr;
  const auto lap0 = std::chrono::steady_clock::now();
  auto lap = [&](const char *what) {
    if (!lap_on) return;
    (void)hipStreamSynchronize(st);
    fprintf(stderr, "[strl_front_treads_named] %s at %.4f s\n", what, std::chrono::duration<double>(std::chrono::steady_clock::now() - lap0).count());
  };
  if ((rc = strl::front_tread_names(c, c->front, c->treads.as<strl_tread>(), c->n_treads_dev, (uint32_t)nt, static_cast<uint64_t *>(p_ref), static_cast<uint32_t *>(p_len),
                                    static_cast<uint64_t *>(p_off), static_cast<uint8_t *>(p_out), ocap, static_cast<uint64_t *>(p_tiles), st)))
    return rc;
  lap("references, offsets and name bytes on the device");
  STRL_HIP(hipMemcpyAsync(treads, c->treads.p, (size_t)nt * sizeof(strl_tread), hipMemcpyDeviceToHost, st));
  uint64_t total = 0;
  STRL_HIP(hipMemcpyAsync(&total, static_cast<uint64_t *>(p_off) + nt, 8, hipMemcpyDeviceToHost, st));
  if (qname_off) STRL_HIP(hipMemcpyAsync(qname_off, p_off, (size_t)(nt + 1) * 8, hipMemcpyDeviceToHost, st));
  STRL_HIP(hipStreamSynchronize(st));
  if (names_need) *names_need = total;
  int ret = STRL_OK;
  if (qname_off && names) {
    if (total > names_cap) { set_error("strl_front_treads_named: %llu bytes of names, capacity %llu", (unsigned long long)total, (unsigned long long)names_cap); ret = STRL_ERR_CAPACITY; }
    else if (total) STRL_HIP(hipMemcpy(names, p_out, (size_t)total, hipMemcpyDeviceToHost));
  }
  lap("treads, offsets and names on the host");
  return ret;
}

}  // extern "C"
