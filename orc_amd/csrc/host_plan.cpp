// Host stream planning (host_plan.hh): the three group parsers, the cut loop
// and the seek lookup. Header arithmetic identical to the device walks.
#include "host_plan.hh"

#include <algorithm>

namespace orcg {

namespace {

const uint8_t kFbs[32] = {1,  2,  3,  4,  5,  6,  7,  8,  9,  10, 11, 12, 13, 14, 15, 16,
                          17, 18, 19, 20, 21, 22, 23, 24, 26, 28, 30, 32, 40, 48, 56, 64};

uint32_t closest_fixed_bits(uint32_t n) {
  if (n == 0) return 1;
  if (n <= 24) return n;
  if (n <= 26) return 26;
  if (n <= 28) return 28;
  if (n <= 30) return 30;
  if (n <= 32) return 32;
  if (n <= 40) return 40;
  if (n <= 48) return 48;
  if (n <= 56) return 56;
  return 64;
}

// End of the varint starting at `p` (one past its terminator), or len + 1
// when the stream ends first.
uint64_t varint_end(const uint8_t* s, uint64_t len, uint64_t p) {
  while (p < len && (s[p] & 0x80u)) ++p;
  return p < len ? p + 1 : len + 1;
}

// The same for a DELTA header's varints: no header byte lies kRlev2HdrLim
// bytes or more past the run's first (parse_run's `lim`, rlev2_device.hh).
uint64_t header_varint_end(const uint8_t* s, uint64_t len, uint64_t pos, uint64_t p) {
  const uint64_t lim = std::min<uint64_t>(len, pos + kRlev2HdrLim);
  while (p < lim && (s[p] & 0x80u)) ++p;
  return p < lim ? p + 1 : len + 1;
}

}  // namespace

uint32_t host_parse_run(const uint8_t* s, uint64_t len, uint64_t pos, uint64_t* run_len, uint64_t* run_end,
                        int java) {
  *run_len = 0;  // a bad run delivers none of its values
  // the run of L values ends at `end`, if the stream holds it whole
  auto whole = [&](uint64_t L, uint64_t end, uint32_t e = kErrNone) -> uint32_t {
    *run_end = end;
    if (end > len) return kErrBadRead;
    if (e == kErrNone) *run_len = L;
    return e;
  };
  const uint32_t fb = s[pos];
  const uint32_t kind = fb >> 6;
  if (kind == 0) return whole((fb & 7) + 3, pos + 2 + ((fb >> 3) & 7));
  if (pos + 2 > len) return kErrBadRead;
  uint64_t L = ((uint64_t)(fb & 1) << 8 | s[pos + 1]) + 1;
  if (kind == 1 || kind == 2) {
    const uint32_t W = kFbs[(fb >> 1) & 0x1f];
    uint64_t data = pos + 2;
    uint32_t cfb = 0, pl = 0;
    if (kind == 2) {
      if (pos + 4 > len) return kErrBadRead;
      const uint32_t third = s[pos + 2], fourth = s[pos + 3];
      const uint32_t bw = (third >> 5) + 1;
      const uint32_t pbs = kFbs[third & 0x1f];
      const uint32_t pgw = (fourth >> 5) + 1;
      pl = fourth & 0x1f;
      if (pl == 0 && !java) return kErrPatchedPl0;
      if (pos + 4 + bw > len) return kErrBadRead;
      data = pos + 4 + bw;
      if (data + (W * L + 7) / 8 > len) return kErrBadRead;
      // Java (RunLengthIntegerReaderV2.java:196-202): with skipCorrupt the
      // list is read at getClosestFixedBits(pw + pgw) bits an entry
      if (pbs + pgw > 64 && java != 2) return java ? kErrJavaCorrupt : kErrPatchedWidth;
      cfb = closest_fixed_bits(pbs + pgw);
    }
    // Java: unpackedPatch[0] of an empty list
    return whole(L, data + (W * L + 7) / 8 + ((uint64_t)cfb * pl + 7) / 8,
                 kind == 2 && pl == 0 ? kErrJavaPatchIndex : kErrNone);
  }
  const uint32_t fbo = (fb >> 1) & 0x1f;
  const uint32_t W = fbo ? kFbs[fbo] : 0;
  uint64_t q = pos + 2;
  for (int k = 0; k < 2; ++k)
    if ((q = header_varint_end(s, len, pos, q)) > len) return kErrBadRead;
  if (W != 0 && L < 2) {
    if (!java) return kErrDeltaLength;
    L = 2;  // Java (:125-145): the first value, first + deltaBase, no deltas
  }
  return whole(L, q + (W ? ((uint64_t)W * (L - 2) + 7) / 8 : 0));
}

uint32_t host_parse_v1_group(const uint8_t* s, uint64_t len, uint64_t pos, uint64_t* count, uint64_t* end, int) {
  const int32_t h = (int32_t)(int8_t)s[pos];
  const uint64_t k = h >= 0 ? 1 : (uint64_t)(-h);  // varints: a run's base, a literal's values
  uint64_t q = pos + (h >= 0 ? 2 : 1), done = 0;
  while (done < k && q <= len && (q = varint_end(s, len, q)) <= len) ++done;
  *end = q;
  if (done < k) {
    *count = h >= 0 ? 0 : done;
    return kErrV1BadRead;
  }
  *count = h >= 0 ? (uint64_t)h + 3 : k;
  return kErrNone;
}

uint32_t host_parse_byte_group(const uint8_t* s, uint64_t len, uint64_t pos, uint64_t* count, uint64_t* end, int) {
  const uint32_t h = s[pos];
  *count = h < 0x80 ? h + 3 : 256 - h;
  *end = pos + (h < 0x80 ? 2 : 1 + *count);
  if (*end <= len) return kErrNone;
  *count = h < 0x80 ? 0 : len - pos - 1;
  return kErrByteBadRead;
}

orcg_rlev2_plan* cut_stream(const uint8_t* src, uint64_t len, uint64_t max_bytes, uint64_t max_values,
                            GroupParser parse, CutAtBad at_bad, int java) {
  auto* p = new orcg_rlev2_plan();
  uint64_t pos = 0, vi = 0, seg_b = 0, seg_v = 0;
  bool open = false;
  while (pos < len) {
    uint64_t n = 0, end = 0;
    const uint32_t e = parse(src, len, pos, &n, &end, java);
    const bool may_cut = e == kErrNone || at_bad == CutAtBad::kAlways || n > 0;
    if (may_cut && (!open || pos - seg_b >= max_bytes || vi - seg_v >= max_values)) {
      p->segs.push_back({pos, vi});
      seg_b = pos;
      seg_v = vi;
      open = true;
    }
    vi += n;
    if (e != kErrNone) {
      p->err = e;
      p->err_at = vi;
      break;
    }
    pos = end;
  }
  p->values = vi;
  return p;
}

uint64_t locate(const orcg_rlev2_plan& plan, const uint8_t* s, uint64_t len, uint64_t rel, GroupParser parse) {
  auto it = std::upper_bound(plan.segs.begin(), plan.segs.end(), rel,
                             [](uint64_t b, const orcg_segment& g) { return b < g.byte_offset; });
  if (it == plan.segs.begin()) return kNotFound;
  --it;
  uint64_t p = it->byte_offset, v = it->value_index;
  while (p < rel && p < len) {
    uint64_t n, end;
    if (parse(s, len, p, &n, &end, 0) != kErrNone) break;
    p = end;
    v += n;
  }
  return p == rel && v <= plan.values ? v : kNotFound;
}

}  // namespace orcg
