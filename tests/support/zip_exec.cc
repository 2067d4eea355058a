// tests/support/zip_exec.cc -- TEST-ONLY driver of rejit_amd/csrc/record_zip.h, compiled with g++ (tests/test_record_zip.py).
// It walks the call the way record_zip.hip's kernels do -- the resolve (every column's row through record_rows.h's resolver,
// the pieces staged, the first bad (row, column) as the largest word), the plan unit by unit (the running sum carried from
// unit to unit where the kernel looks back), the emit chunk by chunk: the chunk's rows from one pair of searches, every row's
// byte-written parts once into the chunk's image (the kernel's LDS), then every aligned group of 16 either streamed from its
// own offset or taken from the image -- with the unit size and the chunk size chosen by the test.  Every access is checked
// against its range, and every output byte, image byte and table row may be written only once; a streamed group must not
// have an image byte written under it.  ze_row_cuts makes one row again at every possible cut and compares with byte_at.
//
// With -DZIP_EXEC_MAIN the file is a stand-alone program (built with -fsanitize=address,undefined by the test): the same driver
// over a fixed case list and seeded ones, against a join written with std::string, over allocations exact in their last byte.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../rejit_amd/csrc/record_zip.h"
#include "checked_image.h"
#include "checked_table.h"
#include "checked_text.h"

using namespace rejit_amd;

namespace {

// record_zip.h's Source over host tables: the staged pieces, the widths, the separator, the texts -- all checked
struct CheckedSource {
  const zip::Column* cols;
  uint32_t n_cols;
  const uint8_t* sep;
  uint64_t sep_len;
  const std::vector<zip::Piece>* stage;
  uint64_t k;
  std::vector<CheckedText> texts;
  mutable bool left_range = false;
  CheckedSource(const zip::Column* cols_, uint32_t n_cols_, const uint8_t* sep_, uint64_t sep_len_, const std::vector<zip::Piece>* stage_, uint64_t k_)
      : cols(cols_), n_cols(n_cols_), sep(sep_), sep_len(sep_len_), stage(stage_), k(k_) {
    for (uint32_t c = 0; c < n_cols; c++) texts.push_back(CheckedText{cols[c].text, cols[c].n});
  }
  zip::Piece piece(uint64_t j, uint32_t c) const {
    if (j >= k || c >= n_cols) {
      left_range = true;
      return zip::Piece{0, 0};
    }
    return (*stage)[j * n_cols + c];
  }
  int32_t width(uint32_t c) const {
    if (c >= n_cols) left_range = true;
    return c < n_cols ? cols[c].width : 0;
  }
  uint32_t sep_byte(uint32_t i) const {
    if (i >= sep_len) left_range = true;
    return i < sep_len ? sep[i] : 0;
  }
  uint32_t text_byte(uint32_t c, uint64_t s) const {
    if (c >= n_cols) {
      left_range = true;
      return 0;
    }
    return texts[c].byte(s);
  }
  void load16(uint32_t c, uint64_t s, uint32_t w[4]) const {
    if (c >= n_cols || s + 16 > cols[c].n) {   // (the device's load16 takes 16 bytes inside the text only)
      left_range = true;
      w[0] = w[1] = w[2] = w[3] = 0;
      return;
    }
    texts[c].load16(s, w);
  }
  bool any_left() const {
    bool left = left_range;
    for (const CheckedText& t : texts) left |= t.left_range;
    return left;
  }
};

// the resolve over every row: the pieces staged, the rows' lengths; -> the first bad word (0: none)
unsigned long long resolve_all(const zip::Column* cols, uint32_t n_cols, uint64_t sep_len, uint64_t k, uint64_t unit, std::vector<zip::Piece>* stage,
                               std::vector<uint64_t>* row_len) {
  unsigned long long worst = 0;
  for (uint64_t u0 = 0; u0 < k; u0 += unit)
    for (uint64_t j = u0; j < k && j < u0 + unit; j++) {
      uint64_t len = 0;
      for (uint32_t c = 0; c < n_cols; c++) {
        const zip::Column& col = cols[c];
        const rows::Row row = rows::resolve(col.rec_begin, col.rec_end, col.indices, col.n_records, col.n, j);
        if (row.bad) {
          const unsigned long long word = zip::bad_word(j, c);
          if (word > worst) worst = word;
          break;
        }
        (*stage)[j * n_cols + c] = zip::Piece{row.rb, row.len()};
        len += zip::field_length(c, row.len(), col.width, sep_len);
      }
      (*row_len)[j] = len;
    }
  return worst;
}

struct Made {
  uint64_t streamed = 0, from_image = 0;
  bool twice = false, left_range = false, used_stream = false;
};

// The output bytes [c0, c1) (c0 a multiple of 16) as the emit makes them from rows [j0, j1): the image (`room` bytes), then
// group by group.  got[i] = byte c0 + i.  ob(j) through `table`.
Made make_chunk(const CheckedSource& src, const pack::View& table, uint64_t j0, uint64_t j1, uint64_t sep_len, uint32_t pad, uint32_t fill, uint64_t c0,
                uint64_t c1, uint64_t room, std::vector<uint8_t>* got) {
  CheckedImage image(room, fill, c0, c1);
  bool any_streamed = false;
  for (uint64_t j = j0; j < j1; j++) {
    const uint64_t at = table.ob_at(j);
    if (at >= c1) continue;
    any_streamed |= zip::row_edges(src, src.n_cols, sep_len, pad, j, at, c0, c1, [&](uint64_t in_image, uint32_t byte) { image.put(in_image, byte); });
  }
  image.store(
      [&](uint64_t p, uint32_t w[4]) {
        if (!any_streamed) return false;
        const uint64_t u = pack::upper_bound(table, j0, j1, p);
        return u > j0 && zip::group_streamed(src, src.n_cols, sep_len, pad, u - 1, table.ob_at(u - 1), p, w);
      },
      got);
  Made m;
  m.streamed = image.streamed, m.from_image = image.from_image, m.used_stream = any_streamed;
  m.twice = image.twice, m.left_range = image.left_range || src.any_left();
  return m;
}

}  // namespace

// [0] kMaxColumns, [1] kMaxSep, [2] kMaxWidth, [3] kStreamBytes, [4] kEmitChunk, [5] sizeof(Column), [6] sizeof(Piece)
extern "C" void ze_constants(int64_t* out) {
  out[0] = zip::kMaxColumns;
  out[1] = zip::kMaxSep;
  out[2] = zip::kMaxWidth;
  out[3] = zip::kStreamBytes;
  out[4] = zip::kEmitChunk;
  out[5] = sizeof(zip::Column);
  out[6] = sizeof(zip::Piece);
}

// the bad word's order: 1 when word(j1, c1) > word(j2, c2) and both decode back
extern "C" int ze_bad_word_before(uint64_t j1, uint32_t c1, uint64_t j2, uint32_t c2) {
  const unsigned long long a = zip::bad_word(j1, c1), b = zip::bad_word(j2, c2);
  if (zip::bad_row_of(a) != j1 || zip::bad_column_of(a) != c1 || zip::bad_row_of(b) != j2 || zip::bad_column_of(b) != c2 || a == 0 || b == 0) return -1;
  return a > b;
}

// summary: [0] total, [1] the first bad row (~0: none), [2] its column, [3] check_call's code, [4] chunks, [5] groups streamed,
// [6] groups from the image, [7] chunks that took the stream tier.  message: 320 bytes for the refusal's text.
// Returns 0; -1 when an access left its range or something was written twice (a bug the kernel would pay for with a fault or a
// race); -2 for a call check_call refuses.
extern "C" long ze_zip(const zip::Column* cols, int n_cols, const char* sep, uint64_t sep_len, int pad, unsigned flags, int fill, uint64_t lead,
                       uint64_t gap, uint64_t unit, uint64_t chunk, uint8_t* out, uint64_t out_cap, uint64_t* out_begin, uint64_t* out_end,
                       uint64_t* summary, char* message) {
  for (int i = 0; i < 8; i++) summary[i] = 0;
  summary[1] = ~0ull;
  message[0] = 0;
  static const char kCall[] = "rj_scan_records_zip";
  const zip::Refusal why = zip::check_call(cols, n_cols, sep, sep_len, pad, flags, fill, lead, gap, out, out_cap, out_begin, out_end);
  summary[3] = why.code;
  const uint64_t k = cols && n_cols >= 1 ? zip::rows_of(cols[0]) : 0;
  if (why.code != zip::kFine) {
    zip::refusal_message(message, 320, kCall, why, k);
    return -2;
  }
  if (unit == 0 || chunk == 0 || chunk % pack::kGroupBytes != 0) return -2;
  const uint32_t C = static_cast<uint32_t>(n_cols);
  // ---- resolve: no table row and no byte behind a bad row
  std::vector<zip::Piece> stage(k * C);
  std::vector<uint64_t> row_len(k);
  const unsigned long long worst = resolve_all(cols, C, sep_len, k, unit, &stage, &row_len);
  if (worst != 0) {
    summary[1] = zip::bad_row_of(worst);
    summary[2] = zip::bad_column_of(worst);
    zip::bad_row_message(message, 320, kCall, worst);
    return 0;
  }
  // ---- plan
  bool twice = false;
  std::vector<uint64_t> own_begin(k + 1);
  uint64_t* ob = out_begin ? out_begin : own_begin.data();
  std::vector<uint8_t> row_once(k, 0);
  uint64_t before = 0;
  for (uint64_t u0 = 0; u0 < k; u0 += unit) {
    uint64_t in_unit = 0;
    for (uint64_t j = u0; j < k && j < u0 + unit; j++) {
      if (row_once[j]) twice = true;
      row_once[j] = 1;
      ob[j] = lead + before + in_unit;
      if (out_end) out_end[j] = ob[j] + row_len[j];
      in_unit += pack::row_advance(false, 0, row_len[j], gap);
    }
    before += in_unit;
  }
  const uint64_t total = lead + before;
  summary[0] = total;
  // ---- emit
  const pack::View table{ob, nullptr, nullptr, nullptr, 0, k, total};
  const CheckedSource src(cols, C, reinterpret_cast<const uint8_t*>(sep), sep_len, &stage, k);
  bool left_range = false;
  const long chunks = walk_chunks(table, k, total, chunk, out, out_cap, [&](uint64_t c0, uint64_t c1, uint64_t j0, uint64_t j1, std::vector<uint8_t>* got) {
    const Made m = make_chunk(src, table, j0, j1, sep_len, static_cast<uint32_t>(pad), static_cast<uint32_t>(fill), c0, c1, chunk, got);
    summary[5] += m.streamed, summary[6] += m.from_image, summary[7] += m.used_stream;
    twice |= m.twice, left_range |= m.left_range;
  });
  if (chunks < 0) return -1;
  summary[4] = static_cast<uint64_t>(chunks);
  return left_range || twice ? -1 : 0;
}

// Row j of the call made again at EVERY cut: for every a in [0, len] the row stands at an ob that puts byte a on a chunk's
// boundary, and the two chunks around it are made as the emit makes them (chunk bytes each side); both halves must equal
// byte_at's bytes.  Returns len, -1: an access left its range or a byte was written twice, -3: a production differs.
extern "C" long ze_row_cuts(const zip::Column* cols, int n_cols, const char* sep, uint64_t sep_len, int pad, uint64_t j, uint8_t* row_out, uint64_t room) {
  const uint32_t C = static_cast<uint32_t>(n_cols);
  const uint64_t k = zip::rows_of(cols[0]);
  std::vector<zip::Piece> stage(k * C);
  std::vector<uint64_t> row_len(k);
  if (resolve_all(cols, C, sep_len, k, 256, &stage, &row_len) != 0 || j >= k) return -2;
  const CheckedSource src(cols, C, reinterpret_cast<const uint8_t*>(sep), sep_len, &stage, k);
  const uint64_t len = zip::row_length(src, C, sep_len, j);
  if (len != row_len[j] || len > room) return -3;
  for (uint64_t i = 0; i < len; i++) row_out[i] = static_cast<uint8_t>(zip::byte_at(src, C, sep_len, static_cast<uint32_t>(pad), j, i));
  const uint64_t chunk = (len + 31) / 16 * 16;   // either side of the cut holds the whole row
  std::vector<uint8_t> got;
  for (uint64_t a = 0; a <= len; a++) {
    const uint64_t boundary = chunk, at = boundary - a;   // ob: byte a of the row is output byte `boundary`
    // a one-row table: ob_at(j) for this j only -- the view's base makes every other row a range error of the vector below
    std::vector<uint64_t> ob(k, ~0ull);
    ob[j] = at;
    const pack::View table{ob.data() + j, nullptr, nullptr, nullptr, j, j + 1, at + len};
    for (int side = 0; side < 2; side++) {
      const uint64_t c0 = side ? boundary : 0, c1 = side ? at + len : boundary;
      if (c0 >= c1) continue;
      const Made m = make_chunk(src, table, j, j + 1, sep_len, static_cast<uint32_t>(pad), 0xEE, c0, c1, 2 * chunk, &got);
      if (m.twice || m.left_range) return -1;
      for (uint64_t q = c0; q < c1; q++) {
        const uint8_t want = q < at ? 0xEE : row_out[q - at];
        if (got[q - c0] != want) return -3;
      }
    }
  }
  return static_cast<long>(len);
}

#ifdef ZIP_EXEC_MAIN
#include <stdio.h>
#include <stdlib.h>

#include <string>

namespace {

struct HostColumn {
  std::vector<uint8_t> text;
  std::vector<uint64_t> begins, ends, indices;
  bool with_indices;
  int32_t width;
};

// a column of n_records records with lengths from `lengths`, packed without slack: the sanitizer sees a read behind the text
HostColumn make_column(uint64_t n_records, const std::vector<uint64_t>& lengths, uint64_t k, bool with_indices, int32_t width) {
  HostColumn h;
  h.with_indices = with_indices, h.width = width;
  for (uint64_t r = 0; r < n_records; r++) {
    const uint64_t len = lengths[rnd(lengths.size())];
    h.begins.push_back(h.text.size());
    for (uint64_t i = 0; i < len; i++) h.text.push_back(static_cast<uint8_t>('a' + (r + 3 * i) % 26));
    h.ends.push_back(h.text.size());
  }
  if (with_indices)
    for (uint64_t j = 0; j < k; j++) h.indices.push_back(rnd(n_records));
  return h;
}

std::string want_row(const std::vector<HostColumn>& hs, const std::string& sep, int pad, uint64_t j) {
  std::string row;
  for (size_t c = 0; c < hs.size(); c++) {
    const HostColumn& h = hs[c];
    const uint64_t r = h.with_indices ? h.indices[j] : j;
    const std::string piece(reinterpret_cast<const char*>(h.text.data()) + h.begins[r], h.ends[r] - h.begins[r]);
    const size_t w = static_cast<size_t>(h.width < 0 ? -h.width : h.width);
    const std::string padding(w > piece.size() ? w - piece.size() : 0, static_cast<char>(pad));
    if (c) row += sep;
    row += h.width > 0 ? padding + piece : piece + padding;
  }
  return row;
}

}  // namespace

int main() {
  const std::vector<std::vector<uint64_t>> length_sets = {{0}, {0, 1, 15, 16, 17, 33}, {31, 32, 33}, {3, 8, 200}, {1, 2, 5000}};
  const int32_t widths[] = {0, 1, -1, 7, -7, 4096, -4096, 40};
  const uint64_t seps[] = {0, 1, 2, 64};
  int cases = 0;
  for (int n_cols : {1, 2, 3, 16})
    for (size_t ls = 0; ls < length_sets.size(); ls++)
      for (int layout = 0; layout < 4; layout++) {
        const uint64_t k = 40 + rnd(30);
        const uint64_t lead = layout & 1 ? 5 : 0, gap = layout == 0 ? 0 : layout == 1 ? 1 : layout == 2 ? 3 : 40;
        const uint64_t sep_len = seps[(ls + layout + n_cols) % 4];
        const int pad = layout == 3 ? '0' : ' ';
        std::string sep;
        for (uint64_t i = 0; i < sep_len; i++) sep += static_cast<char>('A' + i % 26);
        std::vector<HostColumn> hs;
        for (int c = 0; c < n_cols; c++) {
          const bool with_indices = (c + layout) % 2 == 1;
          hs.push_back(make_column(with_indices ? 25 : k, length_sets[ls], k, with_indices, widths[(c + ls + layout) % 8]));
        }
        std::vector<zip::Column> cols;
        for (const HostColumn& h : hs)
          cols.push_back(zip::Column{h.text.data(), h.text.size(), h.begins.data(), h.ends.data(), h.begins.size(), h.with_indices ? h.indices.data() : nullptr,
                                     h.with_indices ? h.indices.size() : 0, h.width, 0});
        std::string want(lead, '\n');
        std::vector<uint64_t> want_begin, want_end;
        for (uint64_t j = 0; j < k; j++) {
          want_begin.push_back(want.size());
          want += want_row(hs, sep, pad, j);
          want_end.push_back(want.size());
          want += std::string(gap, '\n');
        }
        std::vector<uint64_t> ob(k), oe(k);
        uint64_t summary[8];
        char message[320];
        void* room = nullptr;
        if (posix_memalign(&room, 16, want.size() ? want.size() : 1) != 0) return 1;
        uint8_t* out = static_cast<uint8_t*>(room);
        const uint64_t chunk = layout == 0 ? 64 : layout == 1 ? 4096 : 256;
        const long rc = ze_zip(cols.data(), n_cols, sep.data(), sep_len, pad, 0, '\n', lead, gap, 16, chunk, out, want.size(), ob.data(), oe.data(), summary, message);
        const bool same = rc == 0 && summary[0] == want.size() && memcmp(out, want.data(), want.size()) == 0 && ob == want_begin && oe == want_end;
        free(out);
        if (!same) {
          fprintf(stderr, "zip_exec: %d columns, lengths %zu, layout %d: rc %ld total %llu want %zu\n", n_cols, ls, layout, rc,
                  static_cast<unsigned long long>(summary[0]), want.size());
          return 1;
        }
        for (uint64_t j = 0; j < k; j += 13) {   // a row at every cut (the work is quadratic in the row: the short ones here)
          if (want_end[j] - want_begin[j] > 512) continue;
          std::vector<uint8_t> row(want_end[j] - want_begin[j] + 1);
          const long len = ze_row_cuts(cols.data(), n_cols, sep.data(), sep_len, pad, j, row.data(), row.size());
          if (len != static_cast<long>(want_end[j] - want_begin[j]) || memcmp(row.data(), want.data() + want_begin[j], len) != 0) {
            fprintf(stderr, "zip_exec: %d columns, lengths %zu, layout %d, row %llu: cuts %ld\n", n_cols, ls, layout, static_cast<unsigned long long>(j), len);
            return 1;
          }
        }
        cases += static_cast<int>(k);
      }
  printf("zip_exec: %d cases\n", cases);
  return 0;
}
#endif
