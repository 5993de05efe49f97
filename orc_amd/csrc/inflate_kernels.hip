// Snappy (raw block format) decompression of independent chunks on the device:
// the device half of the host's snappy_decompress (orc_file.cpp), with its
// check order and texts (dev_error.hh kErrSnappy*). DESIGN.md §3.11.
// LZ4 (raw blocks) on the same ring, slice and flush:
// lz4_inflate_kernel below.
//
// One wavefront owns one chunk. The decompressed history lives in an LDS ring
// of kSnappyRing bytes: a copy element reads what the elements before it
// wrote, and LDS operations of one wave execute in order, so a chain of
// dependent copies never waits for HBM. The ring is flushed to the output in
// 16-byte stores; ring byte (o + align) & (ring - 1) holds output byte o,
// align = the output address mod 16, so a 16-byte output word is a 16-byte
// ring word. A copy that reaches behind the ring (legal, rare: chunks may be
// 256 KB) reads the output back from HBM after the wave's stores completed.
// Stored ("original") chunks are one literal of the chunk's length.
//
// The input is untrusted. Source bytes come through a range-checked buffer
// descriptor over the chunk (loads past it return zeros) and every decision
// is bounded by the chunk's length; every store is preceded by the host
// decoder's own guard (o + len <= ulen, 0 < off <= o); the ring index is
// masked; a flush writes [flushed, o) of the chunk's output and o <= ulen =
// the table's dst_bytes, which the launcher bounds by the output's length.
#include "device_util.hh"
#include "dev_error.hh"
#include "inflate_plan.hh"
#include "orcg_internal.hh"

namespace orcg {

using namespace dev;

namespace {

constexpr uint32_t kRing = kSnappyRing;
constexpr uint32_t kMask = kRing - 1;
// the ring is flushed once this much is pending; a literal is taken in pieces
constexpr uint32_t kFlush = 16384;
constexpr uint32_t kPiece = 4096;
// bytes the ring must still hold for the next element: the unflushed part
// (< kFlush + kPiece) must not be overwritten by a piece or a copy, and a far
// copy (off > kRing) must find its source flushed
static_assert(kFlush + 2 * kPiece + 64 <= kRing, "the ring holds the unflushed bytes and the next piece");
static_assert((kRing & kMask) == 0 && kFlush % 16 == 0, "power-of-two ring, whole words per flush");

typedef uint32_t iu4 __attribute__((ext_vector_type(4)));

// The chunk's bytes: descriptor byte 0 = the chunk's first byte rounded down
// to 16 (`adj` bytes in front), records to the chunk's end rounded up to a dword.
struct ChunkSrc {
  __amdgpu_buffer_rsrc_t rs;
  uint32_t adj;
};

// 5 source bytes at least from chunk offset p (p < 2^31) on every lane; the
// 256-byte slice [wbase, wbase + 256) of the descriptor is held one dword per
// lane and re-read when p leaves it (p, wbase wave-uniform).
struct Slice {
  uint32_t word;
  uint32_t wbase;
  bool valid;
};

__device__ __forceinline__ uint64_t peek(const ChunkSrc& c, Slice& s, uint32_t p, int lane) {
  const uint32_t q = c.adj + p;  // descriptor-relative: the slice's dwords are aligned
  if (!s.valid || q < s.wbase || q + 8 > s.wbase + 256) {
    s.wbase = q & ~3u;
    s.word = __builtin_amdgcn_raw_buffer_load_b32(c.rs, s.wbase + 4u * (uint32_t)lane, 0, 0);
    s.valid = true;
  }
  const uint32_t i = uni((q - s.wbase) >> 2);  // <= 62
  const uint64_t lo = rdlane(s.word, i), hi = rdlane(s.word, i + 1);
  return ((hi << 32) | lo) >> ((q & 3u) * 8);  // 5 bytes at least
}

// Ring bytes [flushed, upto) -> the output. Not final: upto is rounded down
// to a 16-byte output word (the caller has at least kFlush pending). Returns
// the new flushed count.
__device__ __forceinline__ uint32_t flush(const uint8_t* ring, uint8_t* out, uint32_t align, uint32_t flushed,
                                          uint32_t upto, bool final, int lane) {
  uint32_t f = flushed;
  const uint32_t head = min((16u - ((align + f) & 15u)) & 15u, upto - f);
  if ((uint32_t)lane < head) out[f + lane] = ring[(align + f + lane) & kMask];
  f += head;
  const uint32_t words = (upto - f) >> 4;
  for (uint32_t w = lane; w < words; w += kWave) {
    const uint32_t o = f + 16u * w;
    *(iu4*)(out + o) = *(const iu4*)(ring + ((align + o) & kMask));
  }
  f += 16u * words;
  if (final) {
    if ((uint32_t)lane < upto - f) out[f + lane] = ring[(align + f + lane) & kMask];
    f = upto;
  }
  return f;
}

// LZ4's literal piece: source bytes [p, p + piece) -> the ring bytes of output
// [o, o + piece). Lane l takes source bytes [4l, 4l + 4) of each 256. A copy
// of the loop in snappy_inflate_kernel: called from there, it changed that
// kernel's instruction schedule (DESIGN.md §3.1 has the same with stream_desc).
__device__ __forceinline__ void lz4_literal_piece(const ChunkSrc& c, uint8_t* ring, uint32_t align, uint32_t p,
                                                  uint32_t o, uint32_t piece, int lane) {
  for (uint32_t k = 4u * lane; k < piece; k += 4u * kWave) {
    const uint32_t a = c.adj + p + k;
    const uint32_t w0 = __builtin_amdgcn_raw_buffer_load_b32(c.rs, a & ~3u, 0, 0);
    const uint32_t w1 = __builtin_amdgcn_raw_buffer_load_b32(c.rs, (a & ~3u) + 4u, 0, 0);
    const uint32_t w = (uint32_t)((((uint64_t)w1 << 32) | w0) >> ((a & 3u) * 8));
    const uint32_t r = align + o + k;
    if (k + 4 <= piece && (r & 3u) == 0) {
      *(uint32_t*)(ring + (r & kMask)) = w;
    } else {
      for (uint32_t j = 0; j < 4 && k + j < piece; ++j) ring[(r + j) & kMask] = (uint8_t)(w >> (8 * j));
    }
  }
  asm volatile("" ::: "memory");
}

// LZ4: a match is expanded in steps of kStep bytes, a byte a lane
constexpr uint32_t kStep = kWave;
// the unflushed bytes (< kFlush between steps and pieces) must survive the
// next piece or step; writing output byte x takes the ring byte of x - kRing,
// which no later offset (<= 65,535 < kRing) reaches
static_assert(kLz4Ring == kRing && kLz4Threads == kWave, "one ring, one wavefront");
static_assert(kFlush + kPiece <= kRing && kFlush + kStep <= kRing,
              "the ring holds the unflushed bytes and the next piece or step");
static_assert(65535 < kRing, "every LZ4 offset lies inside the ring");

// The extension bytes of a length (15 in the token): bytes are added until
// one is not 255. False: the chunk ends inside the run, or the length passed
// `room` (what can still fit; len < 2^31 + 255, no wrap). The run may be
// longer than the slice: peek reloads inside it.
__device__ __forceinline__ bool lz4_extend(const ChunkSrc& c, Slice& s, uint32_t& p, uint32_t n, uint32_t& len,
                                           uint32_t room, int lane) {
  for (;;) {
    if (p >= n) return false;
    const uint32_t b = (uint32_t)peek(c, s, p, lane) & 0xffu;
    ++p;
    len += b;
    if (len > room) return false;
    if (b != 255u) return true;
  }
}

}  // namespace

// LZ4 raw blocks: lz4_block_size's rules (inflate_plan.hh), each repeated ahead
// of the store it guards, one code. ulen = the table's dst_bytes plays the
// walk's cap, and the block must end at it exactly. Every offset lies inside
// the ring, so there is no read-back path. A match has no length bound: it is
// expanded kStep bytes a step. In a step every lane reads its history byte
// before any lane writes (one LDS read, then one LDS write, of the wave): with
// off = 65,535 the step's source ring bytes are the ones it writes, shifted by
// one. The output is periodic in off from o - off on, so lane i of a step at
// o reads byte o - off + i % off for off < kStep: the bytes just written, a
// match longer than the ring included (a step k bytes into a match that began
// at o0 reads o0 - off + (k + i) % off: the phase is folded into o). The flush
// check runs between steps as between pieces.
__global__ __launch_bounds__(kLz4Threads) void lz4_inflate_kernel(const uint8_t* __restrict__ src,
                                                                 const orcg_lz4_chunk* __restrict__ table,
                                                                 uint8_t* dst, unsigned long long* err) {
  __shared__ __attribute__((aligned(16))) uint8_t ring[kRing];
  const int lane = threadIdx.x;
  const uint32_t ci = blockIdx.x;
  const orcg_lz4_chunk t = table[ci];
  const uint32_t n = uni((uint32_t)t.src_bytes);  // the launcher bounds both by 2^31
  const uint32_t ulen = uni((uint32_t)t.dst_bytes);
  const uint8_t* csrc = src + uni64(t.src_offset);
  uint8_t* out = dst + uni64(t.dst_offset);
  const uint32_t align = uni((uint32_t)(uintptr_t)out & 15u);

  ChunkSrc c;
  c.adj = uni((uint32_t)(uintptr_t)csrc & 15u);
  c.rs = __builtin_amdgcn_make_buffer_rsrc((void*)(csrc - c.adj), (short)0, (int)((c.adj + n + 3u) & ~3u), 0x00020000);
  Slice s;
  s.valid = false;
  s.word = 0;
  s.wbase = 0;

  uint32_t p = 0, o = 0, flushed = 0;  // o <= ulen throughout
  uint32_t code = kErrNone;
  const bool stored = uni((uint32_t)t.flags & ORCG_LZ4_STORED) != 0;
  if (stored && n != ulen) code = kErrLz4;
  while (code == kErrNone) {
    // the sequence's literal: a stored chunk is one of the chunk's length
    uint32_t lit = n, token = 0;
    if (!stored) {
      if (p >= n) {
        code = kErrLz4;
        break;
      }
      token = (uint32_t)peek(c, s, p, lane) & 0xffu;
      ++p;
      lit = token >> 4;
      if (lit == 15 && !lz4_extend(c, s, p, n, lit, min(n - p, ulen - o), lane)) {
        code = kErrLz4;
        break;
      }
      if (lit > n - p || lit > ulen - o) {
        code = kErrLz4;
        break;
      }
    }
    while (lit) {
      const uint32_t piece = min(lit, kPiece);
      const uint32_t q = c.adj + p;
      if (piece <= kStep && s.valid && q >= s.wbase && q + piece <= s.wbase + 256) {
        // a short literal inside the slice the token came from (the common
        // sequence): a byte a lane out of the lanes' dwords, no trip to memory.
        // Every lane takes part in the exchange; lanes past the piece drop theirs.
        const uint32_t x = q - s.wbase + (uint32_t)lane;
        const uint32_t w = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(x & ~3u), (int)s.word);
        if ((uint32_t)lane < piece) ring[(align + o + lane) & kMask] = (uint8_t)(w >> ((x & 3u) * 8));
        asm volatile("" ::: "memory");
      } else {
        lz4_literal_piece(c, ring, align, p, o, piece, lane);
      }
      p += piece;
      o += piece;
      lit -= piece;
      if (o - flushed >= kFlush) flushed = flush(ring, out, align, flushed, o, false, lane);
    }
    if (p == n) break;  // the block ends with a literal run
    if (n - p < 2) {
      code = kErrLz4;
      break;
    }
    const uint32_t off = (uint32_t)peek(c, s, p, lane) & 0xffffu;
    p += 2;
    uint32_t len = token & 15u;
    if (len == 15 && !lz4_extend(c, s, p, n, len, ulen - o, lane)) {
      code = kErrLz4;
      break;
    }
    len += 4;
    if (off == 0 || off > o || len > ulen - o) {
      code = kErrLz4;
      break;
    }
    const uint32_t k = off >= kStep ? (uint32_t)lane : (uint32_t)lane % off;
    while (len) {
      const uint32_t step = min(len, kStep);
      uint32_t b = 0;
      if ((uint32_t)lane < step) b = ring[(align + o - off + k) & kMask];
      if ((uint32_t)lane < step) ring[(align + o + lane) & kMask] = (uint8_t)b;
      asm volatile("" ::: "memory");
      o += step;
      len -= step;
      if (o - flushed >= kFlush) flushed = flush(ring, out, align, flushed, o, false, lane);
    }
  }
  if (code == kErrNone && o != ulen) code = kErrLz4;
  if (code != kErrNone) {
    if (lane == 0) report(err, ci, code);
    return;
  }
  flush(ring, out, align, flushed, o, true, lane);
}
// (ahead of snappy_inflate_kernel, which stays the unit's last function: its
// piece of the assembly, the unit's trailer included, is the one of before)

__global__ __launch_bounds__(kSnappyThreads) void snappy_inflate_kernel(const uint8_t* __restrict__ src,
                                                                       const orcg_snappy_chunk* __restrict__ table,
                                                                       uint8_t* dst, unsigned long long* err) {
  __shared__ __attribute__((aligned(16))) uint8_t ring[kRing];
  const int lane = threadIdx.x;
  const uint32_t ci = blockIdx.x;
  const orcg_snappy_chunk t = table[ci];
  const uint32_t n = uni((uint32_t)t.src_bytes);     // the launcher bounds both by 2^31
  const uint32_t ulen = uni((uint32_t)t.dst_bytes);
  const uint8_t* csrc = src + uni64(t.src_offset);
  uint8_t* out = dst + uni64(t.dst_offset);
  const uint32_t align = uni((uint32_t)(uintptr_t)out & 15u);

  ChunkSrc c;
  c.adj = uni((uint32_t)(uintptr_t)csrc & 15u);
  c.rs = __builtin_amdgcn_make_buffer_rsrc((void*)(csrc - c.adj), (short)0, (int)((c.adj + n + 3u) & ~3u), 0x00020000);
  Slice s;
  s.valid = false;
  s.word = 0;
  s.wbase = 0;

  uint32_t p = 0, o = 0, flushed = 0;
  uint32_t code = kErrNone;
  // one pending literal: a stored chunk is one of the chunk's length
  uint32_t lit = 0;
  const bool stored = uni((uint32_t)t.flags & ORCG_SNAPPY_STORED) != 0;
  if (stored) {
    lit = n;
    if (n != ulen) code = kErrSnappyLength;
  } else {
    // the preamble the plan read: its value is the table's dst_bytes
    uint64_t v = 0;
    bool ok = false;
    for (int sh = 0; sh <= 35 && p < n; sh += 7) {
      const uint32_t b = (uint32_t)peek(c, s, p, lane) & 0xffu;
      ++p;
      v |= (uint64_t)(b & 0x7fu) << sh;
      if (!(b & 0x80u)) {
        ok = true;
        break;
      }
    }
    if (!ok || v != ulen) code = kErrSnappyLength;
  }

  while (code == kErrNone && (lit || p < n)) {
    if (lit == 0) {
      const uint64_t h = peek(c, s, p, lane);
      const uint32_t tag = (uint32_t)h & 0xffu;
      const uint32_t kind = tag & 3u;
      ++p;
      if (kind == 0) {
        uint64_t len = (tag >> 2) + 1u;
        if (len > 60) {
          const uint32_t nb = (uint32_t)len - 60;
          if (n - p < nb) {
            code = kErrSnappyLiteralTruncated;
            break;
          }
          len = ((h >> 8) & (0xffffffffull >> (8 * (4 - nb)))) + 1;
          p += nb;
        }
        if ((uint64_t)(n - p) < len || (uint64_t)o + len > ulen) {
          code = kErrSnappyLiteralRange;
          break;
        }
        lit = (uint32_t)len;
      } else {
        uint32_t len, off;
        if (kind == 1) {
          if (p >= n) {
            code = kErrSnappyCopyTruncated;
            break;
          }
          len = 4 + ((tag >> 2) & 7u);
          off = ((tag >> 5) << 8) | ((uint32_t)(h >> 8) & 0xffu);
          p += 1;
        } else if (kind == 2) {
          if (n - p < 2) {
            code = kErrSnappyCopyTruncated;
            break;
          }
          len = 1 + (tag >> 2);
          off = (uint32_t)(h >> 8) & 0xffffu;
          p += 2;
        } else {
          if (n - p < 4) {
            code = kErrSnappyCopyTruncated;
            break;
          }
          len = 1 + (tag >> 2);
          off = (uint32_t)(h >> 8);
          p += 4;
        }
        if (off == 0 || off > o || (uint64_t)o + len > ulen) {
          code = kErrSnappyCopyRange;
          break;
        }
        // len <= 64: one step. Lane i takes history byte o - off + i % off.
        uint32_t b = 0;
        if (off <= kRing) {
          const uint32_t k = off >= len ? (uint32_t)lane : (uint32_t)lane % off;
          if ((uint32_t)lane < len) b = ring[(align + o - off + k) & kMask];
        } else {
          // behind the ring: those bytes are flushed (off > kRing > the
          // pending bytes + 64); the wave's stores must have completed, and
          // the load must stay below them (the asm's memory clobber). One
          // workgroup owns the chunk: its CU's L1 is written through.
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
          if ((uint32_t)lane < len) b = out[o - off + lane];
        }
        if ((uint32_t)lane < len) ring[(align + o + lane) & kMask] = (uint8_t)b;
        asm volatile("" ::: "memory");
        o += len;
      }
    } else {
      // a literal piece: lane l takes source bytes [4l, 4l + 4) of each 256
      uint32_t piece = min(lit, kPiece);
      for (uint32_t k = 4u * lane; k < piece; k += 4u * kWave) {
        const uint32_t a = c.adj + p + k;
        const uint32_t w0 = __builtin_amdgcn_raw_buffer_load_b32(c.rs, a & ~3u, 0, 0);
        const uint32_t w1 = __builtin_amdgcn_raw_buffer_load_b32(c.rs, (a & ~3u) + 4u, 0, 0);
        const uint32_t w = (uint32_t)((((uint64_t)w1 << 32) | w0) >> ((a & 3u) * 8));
        const uint32_t r = align + o + k;
        if (k + 4 <= piece && (r & 3u) == 0) {
          *(uint32_t*)(ring + (r & kMask)) = w;
        } else {
          for (uint32_t j = 0; j < 4 && k + j < piece; ++j) ring[(r + j) & kMask] = (uint8_t)(w >> (8 * j));
        }
      }
      asm volatile("" ::: "memory");
      p += piece;
      o += piece;
      lit -= piece;
    }
    if (o - flushed >= kFlush) flushed = flush(ring, out, align, flushed, o, false, lane);
  }
  if (code == kErrNone && o != ulen) code = kErrSnappyLength;
  if (code != kErrNone) {
    if (lane == 0) report(err, ci, code);
    return;
  }
  flush(ring, out, align, flushed, o, true, lane);
}

int launch_snappy_inflate(Ctx* ctx, const uint8_t* d_src, const orcg_snappy_chunk* d_table, uint64_t nchunks,
                          uint8_t* d_dst, unsigned long long* d_err) {
  if (nchunks == 0) return ORCG_OK;
  if (nchunks > 0x7fffffffull) return set_error(ctx, ORCG_INVALID_ARGUMENT, "too many chunks");
  hipLaunchKernelGGL(snappy_inflate_kernel, dim3((unsigned)nchunks), dim3(kSnappyThreads), 0, ctx->stream, d_src,
                     d_table, d_dst, d_err ? d_err : ctx->d_err);
  return hip_check(ctx, hipGetLastError(), "snappy_inflate_kernel launch");
}

int launch_lz4_inflate(Ctx* ctx, const uint8_t* d_src, const orcg_lz4_chunk* d_table, uint64_t nchunks, uint8_t* d_dst,
                       unsigned long long* d_err) {
  if (nchunks == 0) return ORCG_OK;
  if (nchunks > 0x7fffffffull) return set_error(ctx, ORCG_INVALID_ARGUMENT, "too many chunks");
  hipLaunchKernelGGL(lz4_inflate_kernel, dim3((unsigned)nchunks), dim3(kLz4Threads), 0, ctx->stream, d_src, d_table,
                     d_dst, d_err ? d_err : ctx->d_err);
  return hip_check(ctx, hipGetLastError(), "lz4_inflate_kernel launch");
}

}  // namespace orcg
