// tests/support/plane_args_exec.cc -- rejit_amd/csrc/plane_args.h behind a C interface for tests/test_plane_args.py, and
// (-DPLANE_ARGS_EXEC_MAIN) as a stand-alone program that sweeps the same functions against brute force on small texts:
// what the test builds under the address and undefined-behaviour sanitizers.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../rejit_amd/csrc/plane_args.h"

using namespace rejit_amd;

constexpr uint32_t kRows = 12;  // kPlaneMaxBases (kernels.h)

extern "C" {

// base: [kRows][8] bytes; lo / hi / idx: [kRows][8] words (lo / hi as PlaneGParams takes them: all kRows rows)
void pa_encodings(const uint8_t* base, uint32_t n_bases, uint32_t code_shift, uint32_t n_cmp, uint32_t* lo, uint32_t* hi, uint32_t* mask_bits,
                  uint32_t* idx) {
  const uint8_t(*b)[8] = reinterpret_cast<const uint8_t(*)[8]>(base);
  plane_masks(b, n_bases, code_shift, kRows, reinterpret_cast<uint32_t(*)[8]>(lo), reinterpret_cast<uint32_t(*)[8]>(hi));
  *mask_bits = plane_mask_bits(b, n_bases, code_shift);
  plane_idx(b, n_bases, code_shift, n_cmp, kRows, reinterpret_cast<uint32_t(*)[8]>(idx));
}

// out: wlo, whi, first_block, end_block
void pa_blocks(uint64_t n, uint64_t sb, uint64_t se, uint32_t min_offset, uint32_t max_offset, uint32_t n_cmp, uint64_t* out) {
  const PlaneBlocks r = plane_blocks(n, sb, se, min_offset, max_offset, n_cmp);
  out[0] = r.wlo;
  out[1] = r.whi;
  out[2] = r.first_block;
  out[3] = r.end_block;
}

// out: span_blocks, span_extra, span_pairs
void pa_split(uint64_t first_block, uint64_t end_block, uint32_t n_regions, uint64_t* out) {
  PlaneBlocks r;
  r.first_block = first_block;
  r.end_block = end_block;
  uint32_t extra = 0;
  plane_split(r.blocks(), n_regions, &out[0], &extra);
  out[1] = extra;
  out[2] = r.span_pairs(n_regions);
}

void pa_window_range(uint64_t n, uint64_t sb, uint64_t se, uint32_t win_offset, uint32_t win_len, uint64_t* out) {
  window_range(n, sb, se, win_offset, win_len, &out[0], &out[1]);
}

// out: wlo, whi, first_chunk, end_chunk
void pa_chunk_range(uint64_t n, uint64_t sb, uint64_t se, int windows, uint32_t min_offset, uint32_t max_offset, uint32_t win_len, int behind,
                    uint64_t* out) {
  const ChunkRange r = chunk_range(n, sb, se, windows != 0, min_offset, max_offset, win_len, behind != 0);
  out[0] = r.wlo;
  out[1] = r.whi;
  out[2] = r.first_chunk;
  out[3] = r.end_chunk;
}

}  // extern "C"

#ifdef PLANE_ARGS_EXEC_MAIN
#define CHECK(c)                                                     \
  do {                                                               \
    if (!(c)) {                                                      \
      std::printf("line %d: %s (case %ld)\n", __LINE__, #c, cases);  \
      return 1;                                                      \
    }                                                                \
  } while (0)

int main() {
  long cases = 0;
  uint32_t seed = 12345;
  auto rnd = [&] { return (seed = seed * 1664525u + 1013904223u) >> 8; };
  for (uint32_t n_bases = 1; n_bases <= kRows; n_bases++)
    for (uint32_t shift = 0; shift <= 6; shift++)
      for (uint32_t n_cmp = 4; n_cmp <= 8; n_cmp++, cases++) {
        uint8_t base[kRows][8];
        for (auto& row : base)
          for (uint8_t& c : row) c = static_cast<uint8_t>(rnd());
        uint32_t lo[kRows][8], hi[kRows][8], idx[kRows][8], bits = 0;
        pa_encodings(&base[0][0], n_bases, shift, n_cmp, &lo[0][0], &hi[0][0], &bits, &idx[0][0]);
        for (uint32_t b = 0; b < kRows; b++)
          for (uint32_t i = 0; i < 8; i++) {
            const uint32_t code = (base[b < n_bases ? b : 0][i] >> shift) & 3u;
            CHECK(lo[b][i] == ((code & 1u) ? 0u : ~0u) && hi[b][i] == ((code & 2u) ? 0u : ~0u));
            CHECK(idx[b][i] == (i < n_cmp ? code : 4u));
            if (b < 2) CHECK(((bits >> (16 * b + 2 * i)) & 3u) == (~code & 3u));
          }
      }
  const uint64_t sizes[] = {0, 7, 8, 15, 16, 2047, 2048, 2049, 4096 + 5};
  const uint32_t offs[] = {0, 3, 7}, regions[] = {1, 2, 7, 64};
  for (uint64_t n : sizes) {
    const uint64_t at[] = {0, 1, 2047, 2048, 2049, n > 0 ? n - 1 : 0, n, n + 1};
    for (uint64_t sb : at)
      for (uint64_t se : at)
        for (uint32_t lo_off : offs)
          for (uint32_t hi_off : offs)
            for (uint32_t n_cmp = 4; n_cmp <= 8; n_cmp += 4, cases++) {
              if (sb >= se || se > n + 1 || hi_off < lo_off) continue;   // (callers answer an empty [sb, se) themselves)
              uint64_t o[4];
              pa_blocks(n, sb, se, lo_off, hi_off, n_cmp, o);
              // brute force: the blocks with a window position w = s + off, s in [sb, se), that has n_cmp bytes of text
              std::vector<char> has(n / 2048 + 2, 0);
              uint64_t any = 0;
              for (uint64_t s = sb; s < se; s++)
                for (uint32_t off = lo_off; off <= hi_off; off++)
                  if (s + off + n_cmp <= n) has[(s + off) / 2048] = 1, any++;
              for (uint64_t b = 0; b < has.size(); b++) CHECK((has[b] != 0) == (b >= o[2] && b < o[3]));
              if (!any) CHECK(o[3] == o[2]);
              for (uint32_t nr : regions) {
                uint64_t sp[3], sum = 0;
                pa_split(o[2], o[3], nr, sp);
                for (uint32_t r = 0; r < nr; r++) sum += sp[0] + (r < sp[1] ? 1 : 0);
                CHECK(sum == o[3] - o[2] && sp[2] >= 1 && sp[2] * nr >= sum && (sp[2] - 1) * nr < sum + (sum == 0));
              }
              if (lo_off == hi_off) {
                uint64_t w[2];
                pa_window_range(n, sb, se, lo_off, n_cmp, w);
                uint64_t first = ~0ull, count = 0;
                for (uint64_t s = sb; s < se; s++)
                  if (s + lo_off + n_cmp <= n) first = count++ ? first : s + lo_off;
                CHECK(w[1] >= w[0] && w[1] - w[0] == count && (count == 0 || w[0] == first));
              }
            }
  }
  // the engine's chunk range: fixed (lo_off == hi_off), floating, behind and dense, against the window positions w = s + off
  // (behind: any w >= sb + lo_off) that have w_len bytes of text, and the 1-KiB chunks that hold them / the starts
  const uint64_t small[] = {0, 3, 8, 1023, 1024, 1025, 2048 + 7, 3 * 1024 + 1};
  long with_positions = 0;
  for (uint64_t n : small) {
    const uint64_t at[] = {0, 1, 1016, 1023, 1024, 1025, 2047, 2048, n > 0 ? n - 1 : 0, n, n + 1};
    for (uint64_t sb : at)
      for (uint64_t se : at)
        for (uint32_t lo_off : offs)
          for (uint32_t hi_off : offs)
            for (uint32_t w_len = 1; w_len <= 8; w_len += 7)
              for (int form = 0; form < 3; form++, cases++) {   // 0 windows, 1 windows behind a prefix, 2 dense
                if (sb >= se || se > n + 1 || hi_off < lo_off) continue;
                uint64_t o[4];
                pa_chunk_range(n, sb, se, form != 2, lo_off, hi_off, w_len, form == 1, o);
                uint64_t first = ~0ull, last = 0, count = 0;
                if (form == 2) {
                  first = sb, last = se - 1, count = se - sb;
                  CHECK(o[0] == 0 && o[1] == 0);
                } else {
                  for (uint64_t w = sb + lo_off; w + w_len <= n; w++)
                    if (form == 1 || w < se + hi_off) first = count++ ? first : w, last = w;
                  CHECK(o[0] == sb + lo_off && o[1] >= o[0] && o[1] - o[0] == count);
                }
                // every position has its chunk, no chunk in front of the first position's or behind the last one's
                if (count) {
                  CHECK(o[2] == first / 1024 && o[3] == last / 1024 + 1);
                  with_positions++;
                } else {
                  CHECK(o[3] <= o[2] + 1 && o[2] == o[0] / 1024);
                }
              }
  }
  CHECK(with_positions > 1000);
  std::printf("%ld cases\n", cases);
  return 0;
}
#endif
