// tests/support/csv_format_exec.cc -- TEST-ONLY driver of rejit_amd/csrc/record_csv_format.h, compiled with g++
// (tests/test_record_csv_format.py).  It walks the call the way record_csv_format.hip's kernels do -- the classify (every
// column's row through record_rows.h's resolver, a short piece by one lane, a long one by the 64 lanes of a wave, the pieces
// staged as their 16 bytes, the first bad (row, column) as the largest word), the plan unit by unit, the emit chunk by chunk:
// the chunk's rows from one pair of searches, every row's byte-written parts once into the chunk's image, the listed expanding
// pieces walked 64 lanes x 16 bytes a step from their begin or from the chunk's checkpoint (the walk between the plan and the
// emit leaves one for every chunk that begins inside a long expanding piece; an entry may be written once, and read only when
// written), then every aligned group of 16 either streamed from its own offset or taken from
// the image -- with the unit size and the chunk size chosen by the test.  Every access is checked against its range, and every
// output byte, image byte and table row may be written only once; a streamed group must not have an image byte written under
// it.  cfe_row_cuts makes one row again at every possible cut and compares with byte_at.
//
// With -DCSV_FORMAT_EXEC_MAIN the file is a stand-alone program (built with -fsanitize=address,undefined by the test): the same
// driver over seeded cases, against a writer written with std::string, over allocations exact in their last byte.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../rejit_amd/csrc/record_csv_format.h"
#include "checked_image.h"
#include "checked_table.h"
#include "checked_text.h"

using namespace rejit_amd;

namespace {

struct CheckedSource {
  const csvf::Column* cols;
  uint32_t n_cols;
  const std::vector<csvf::Staged>* stage;
  uint64_t k;
  std::vector<CheckedText> texts;
  mutable bool left_range = false;
  CheckedSource(const csvf::Column* cols_, uint32_t n_cols_, const std::vector<csvf::Staged>* stage_, uint64_t k_)
      : cols(cols_), n_cols(n_cols_), stage(stage_), k(k_) {
    for (uint32_t c = 0; c < n_cols; c++) texts.push_back(CheckedText{cols[c].text, cols[c].n});
  }
  csvf::Piece piece(uint64_t j, uint32_t c) const {
    if (j >= k || c >= n_cols) {
      left_range = true;
      return csvf::Piece{0, 0, 0, false};
    }
    return csvf::staged_piece((*stage)[j * n_cols + c]);
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

struct Counts {
  uint64_t quoted = 0, doubled = 0, by_wave = 0;
  bool left_range = false;
};

// the classify over every row: the pieces staged, the rows' lengths; -> the first bad word (0: none)
unsigned long long classify_all(const csvf::Column* cols, uint32_t n_cols, uint32_t d, uint32_t q, uint32_t always_mask, uint32_t raw_mask, uint64_t k,
                                uint64_t unit, std::vector<csvf::Staged>* stage, std::vector<uint64_t>* row_len, Counts* counts) {
  unsigned long long worst = 0;
  for (uint64_t u0 = 0; u0 < k; u0 += unit)
    for (uint64_t j = u0; j < k && j < u0 + unit; j++) {
      uint64_t len = 0;
      for (uint32_t c = 0; c < n_cols; c++) {
        const csvf::Column& col = cols[c];
        const rows::Row row = rows::resolve(col.rec_begin, col.rec_end, col.indices, col.n_records, col.n, j);
        if (row.bad) {
          const unsigned long long word = zip::bad_word(j, c);
          if (word > worst) worst = word;
          break;
        }
        const CheckedText text{col.text, col.n};
        bool special = false;
        uint64_t quotes = 0;
        if (row.len() < csvf::kWaveBytes) {
          csvf::classify_groups(text, col.n, row.rb, row.len(), 0, 1, d, q, &special, &quotes);
        } else {   // the wave: lane by lane, then the ballot and the sum
          counts->by_wave++;
          for (uint64_t lane = 0; lane < csv::kLanes; lane++) {
            bool sp = false;
            uint64_t qs = 0;
            csvf::classify_groups(text, col.n, row.rb, row.len(), lane, csv::kLanes, d, q, &sp, &qs);
            special |= sp, quotes += qs;
          }
        }
        counts->left_range |= text.left_range;
        const csvf::Piece pc{row.rb, row.len(), quotes, csvf::need_quotes(n_cols, always_mask, c, row.len(), special)};
        const bool raw = csvf::is_raw(raw_mask, c);
        (*stage)[j * n_cols + c] = csvf::stage_piece(pc);
        const csvf::Piece back = csvf::staged_piece((*stage)[j * n_cols + c]);
        if (back.src != pc.src || back.len != pc.len || back.quotes != pc.quotes || back.need != pc.need) counts->left_range = true;
        len += csvf::field_length(c, pc, raw);
        counts->quoted += pc.need ? 1 : 0;
        counts->doubled += csvf::doubles(pc, raw) ? quotes : 0;
      }
      (*row_len)[j] = len;
    }
  return worst;
}

// one step of the expand walk as the 64 lanes of a wave see it
struct WaveStep {
  uint32_t w[64][4], valid[64], qbits[64], through[64], in_step;
  WaveStep(const CheckedText& text, const csvf::Piece& pc, uint64_t s, uint32_t q) {
    in_step = 0;
    for (uint32_t lane = 0; lane < 64; lane++) {
      const uint64_t g = s + lane * rows::kGroupBytes;
      valid[lane] = g >= pc.len ? 0u : pc.len - g < rows::kGroupBytes ? static_cast<uint32_t>(pc.len - g) : 16u;
      w[lane][0] = w[lane][1] = w[lane][2] = w[lane][3] = 0;
      if (valid[lane]) rows::load_at(text, text.n, pc.src + g, w[lane]);
      qbits[lane] = valid[lane] ? csvf::quote_bits(w[lane], valid[lane], q) : 0u;
      in_step += csv::popcount(qbits[lane]);
      through[lane] = in_step;
    }
  }
};

// the checkpoints of a call: one entry per chunk, written once at the most, read only when written
struct Checkpoints {
  std::vector<csvf::Checkpoint> at;
  std::vector<uint8_t> written;
  bool twice = false, unwritten = false, left_range = false;
  uint64_t steps = 0;
};

// The walk between the plan and the emit: rows [j_begin, j_end) one by one, every checkpointed piece once, an entry for every chunk that begins inside
// it (below `limit`).
void checkpoint_all(const CheckedSource& src, const pack::View& table, uint64_t j_begin, uint64_t j_end, uint32_t q, uint32_t raw_mask, uint64_t chunk, uint64_t limit, Checkpoints* cps) {
  cps->at.assign((limit + chunk - 1) / chunk, csvf::Checkpoint{~0ull, ~0ull});
  cps->written.assign(cps->at.size(), 0);
  for (uint64_t j = j_begin; j < j_end; j++) {
    uint64_t at = table.ob_at(j);
    for (uint32_t c = 0; c < src.n_cols; c++) {
      const csvf::Piece pc = src.piece(j, c);
      const bool raw = csvf::is_raw(raw_mask, c);
      const csvf::Field f = csvf::field_at(at, c, pc, raw);
      at = f.end;
      if (!csvf::checkpointed(pc, raw) || f.data0 >= limit) continue;
      uint64_t before = 0;
      for (uint64_t s = 0; s < pc.len; s += csvf::kWaveStep) {
        const uint64_t step_out = f.data0 + s + before;
        if (step_out >= limit) break;
        cps->steps++;
        const WaveStep st(src.texts[c], pc, s, q);
        const uint64_t step_bytes = pc.len - s < csvf::kWaveStep ? pc.len - s : csvf::kWaveStep;
        const uint64_t step_end = step_out + step_bytes + st.in_step;
        for (uint64_t b = csvf::boundary_from(step_out, chunk); b < step_end && b < limit; b += chunk) {   // (the kernel's chunk: one at the most)
          if (b / chunk >= cps->at.size()) {
            cps->left_range = true;
            continue;
          }
          if (cps->written[b / chunk]) cps->twice = true;
          cps->written[b / chunk] = 1;
          cps->at[b / chunk] = csvf::Checkpoint{s, before};
        }
        before += st.in_step;
      }
    }
  }
}

struct Made {
  uint64_t streamed = 0, from_image = 0, expanded = 0, rewalked = 0;
  bool twice = false, left_range = false, used_stream = false;
};

// The output bytes [c0, c1) (c0 a multiple of 16) as the emit makes them from rows [j0, j1): the image, then group by group.
Made make_chunk(const CheckedSource& src, const pack::View& table, uint64_t j0, uint64_t j1, uint32_t d, uint32_t q, uint32_t raw_mask, uint32_t fill,
                uint64_t c0, uint64_t c1, uint64_t chunk, Checkpoints* cps, std::vector<uint8_t>* got) {
  Made m;
  CheckedImage image(chunk, fill, c0, c1);
  const auto put = [&](uint64_t in_image, uint32_t byte) { image.put(in_image, byte); };
  struct Listed {
    uint64_t j, data0;
    uint32_t c;
  };
  std::vector<Listed> list;
  bool any_streamed = false;
  for (uint64_t j = j0; j < j1; j++) {
    const uint64_t at = table.ob_at(j);
    if (at >= c1) continue;
    any_streamed |= csvf::row_edges(src, src.n_cols, d, q, raw_mask, j, at, c0, c1, put,
                                    [&](uint64_t row, uint32_t col, uint64_t data0) { list.push_back(Listed{row, data0, col}); });
  }
  if (chunk <= csvf::kEmitChunk && list.size() > csvf::kMaxExpand) m.left_range = true;   // the kernel's list would overflow
  // ---- expand: a wave per listed piece, 64 lanes x 16 bytes a step
  for (const Listed& it : list) {
    m.expanded++;
    const csvf::Piece pc = src.piece(it.j, it.c);
    const CheckedText& text = src.texts[it.c];
    csvf::Checkpoint from{0, 0};
    if (csvf::resumes(pc, csvf::is_raw(raw_mask, it.c), it.data0, c0)) {
      const uint64_t entry = c0 / chunk;
      if (c0 % chunk != 0 || entry >= cps->at.size() || !cps->written[entry]) {
        cps->unwritten = true;
      } else {
        from = cps->at[entry];
      }
    }
    uint64_t before = from.before;
    for (uint64_t s = from.s; s < pc.len; s += csvf::kWaveStep) {
      const uint64_t step_out = it.data0 + s + before;
      if (step_out >= c1) break;
      const WaveStep st(text, pc, s, q);
      const uint64_t step_bytes = pc.len - s < csvf::kWaveStep ? pc.len - s : csvf::kWaveStep;
      if (step_out + step_bytes + st.in_step > c0) {
        for (uint32_t lane = 0; lane < 64; lane++)
          if (st.valid[lane])
            csvf::expand_group(st.w[lane], st.valid[lane], st.qbits[lane], q, step_out + lane * rows::kGroupBytes + (st.through[lane] - csv::popcount(st.qbits[lane])),
                               c0, c1, put);
      } else {
        m.rewalked++;
      }
      before += st.in_step;
    }
  }
  image.store(
      [&](uint64_t p, uint32_t w[4]) {
        if (!any_streamed) return false;
        const uint64_t u = pack::upper_bound(table, j0, j1, p);
        return u > j0 && csvf::group_streamed(src, src.n_cols, raw_mask, u - 1, table.ob_at(u - 1), p, w);
      },
      got);
  m.streamed = image.streamed, m.from_image = image.from_image, m.used_stream = any_streamed;
  m.twice |= image.twice, m.left_range |= image.left_range || src.any_left();
  return m;
}

}  // namespace

// [0] kMaxColumns, [1] kStreamBytes, [2] kEmitChunk, [3] kWaveStep, [4] kWaveBytes, [5] kMaxExpand, [6] sizeof(Column), [7] sizeof(Staged),
// [8] kCheckpointBytes
extern "C" void cfe_constants(int64_t* out) {
  out[0] = csvf::kMaxColumns;
  out[1] = csvf::kStreamBytes;
  out[2] = csvf::kEmitChunk;
  out[3] = csvf::kWaveStep;
  out[4] = csvf::kWaveBytes;
  out[5] = csvf::kMaxExpand;
  out[6] = sizeof(csvf::Column);
  out[7] = sizeof(csvf::Staged);
  out[8] = csvf::kCheckpointBytes;
}

// the staged 16 bytes: 1 when (src, len, quotes, need) come back as they went in
extern "C" int cfe_stage_round_trip(uint64_t src, uint64_t len, uint64_t quotes, int need) {
  const csvf::Piece back = csvf::staged_piece(csvf::stage_piece(csvf::Piece{src, len, quotes, need != 0}));
  return back.src == src && back.len == len && back.quotes == quotes && back.need == (need != 0);
}

// summary: [0] total, [1] the first bad row (~0: none), [2] its column, [3] check_call's code, [4] chunks, [5] groups streamed,
// [6] groups from the image, [7] pieces expanded (per chunk), [8] n_quoted, [9] n_doubled, [10] pieces classified by the wave,
// [11] wave steps of the emit that only counted, [12] wave steps of the checkpoint walk.  message: 320 bytes for the refusal's text.
// Returns 0; -1 when an access left its range or something was written twice; -2 for a call check_call refuses.
extern "C" long cfe_format(const csvf::Column* cols, int n_cols, int delimiter, int quote, uint32_t always_mask, uint32_t raw_mask, unsigned flags, int fill,
                           uint64_t lead, uint64_t gap, uint64_t unit, uint64_t chunk, uint8_t* out, uint64_t out_cap, uint64_t* out_begin, uint64_t* out_end,
                           uint64_t* summary, char* message) {
  for (int i = 0; i < 13; i++) summary[i] = 0;
  summary[1] = ~0ull;
  message[0] = 0;
  static const char kCall[] = "rj_scan_records_format_csv";
  const csvf::Refusal why = csvf::check_call(cols, n_cols, delimiter, quote, always_mask, raw_mask, flags, fill, lead, gap, out, out_cap, out_begin, out_end);
  summary[3] = why.code;
  const uint64_t k = cols && n_cols >= 1 ? zip::rows_of(cols[0]) : 0;
  if (why.code != csvf::kFine) {
    csvf::refusal_message(message, 320, kCall, why, k, n_cols);
    return -2;
  }
  if (unit == 0 || chunk == 0 || chunk % pack::kGroupBytes != 0) return -2;
  const uint32_t C = static_cast<uint32_t>(n_cols), d = static_cast<uint32_t>(delimiter), q = static_cast<uint32_t>(quote);
  // ---- classify: no table row and no byte behind a bad row
  std::vector<csvf::Staged> stage(k * C);
  std::vector<uint64_t> row_len(k);
  Counts counts;
  const unsigned long long worst = classify_all(cols, C, d, q, always_mask, raw_mask, k, unit, &stage, &row_len, &counts);
  if (worst != 0) {
    summary[1] = zip::bad_row_of(worst);
    summary[2] = zip::bad_column_of(worst);
    csvf::bad_row_message(message, 320, kCall, worst);
    return 0;
  }
  summary[8] = counts.quoted, summary[9] = counts.doubled, summary[10] = counts.by_wave;
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
  const uint64_t limit = total < out_cap ? total : out_cap;
  const pack::View table{ob, nullptr, nullptr, nullptr, 0, k, total};
  const CheckedSource src(cols, C, &stage, k);
  bool left_range = counts.left_range;
  Checkpoints cps;
  checkpoint_all(src, table, 0, k, q, raw_mask, chunk, limit, &cps);
  summary[12] = cps.steps;
  const long chunks = walk_chunks(table, k, total, chunk, out, out_cap, [&](uint64_t c0, uint64_t c1, uint64_t j0, uint64_t j1, std::vector<uint8_t>* got) {
    const Made m = make_chunk(src, table, j0, j1, d, q, raw_mask, static_cast<uint32_t>(fill), c0, c1, chunk, &cps, got);
    summary[5] += m.streamed, summary[6] += m.from_image, summary[7] += m.expanded, summary[11] += m.rewalked;
    twice |= m.twice, left_range |= m.left_range;
  });
  if (chunks < 0) return -1;
  summary[4] = static_cast<uint64_t>(chunks);
  return left_range || twice || cps.twice || cps.unwritten || cps.left_range ? -1 : 0;
}

// Row j of the call made again at EVERY cut: for every a in [0, len] the row stands at an ob that puts byte a on a chunk's
// boundary, and the two chunks around it are made as the emit makes them; both halves must equal byte_at's bytes.  Returns
// len, -1: an access left its range or a byte was written twice, -3: a production differs.
extern "C" long cfe_row_cuts(const csvf::Column* cols, int n_cols, int delimiter, int quote, uint32_t always_mask, uint32_t raw_mask, uint64_t j, uint8_t* row_out,
                             uint64_t room) {
  const uint32_t C = static_cast<uint32_t>(n_cols), d = static_cast<uint32_t>(delimiter), q = static_cast<uint32_t>(quote);
  const uint64_t k = zip::rows_of(cols[0]);
  std::vector<csvf::Staged> stage(k * C);
  std::vector<uint64_t> row_len(k);
  Counts counts;
  if (classify_all(cols, C, d, q, always_mask, raw_mask, k, 256, &stage, &row_len, &counts) != 0 || j >= k) return -2;
  const CheckedSource src(cols, C, &stage, k);
  const uint64_t len = csvf::row_length(src, C, raw_mask, j);
  if (len != row_len[j] || len > room) return -3;
  for (uint64_t i = 0; i < len; i++) row_out[i] = static_cast<uint8_t>(csvf::byte_at(src, C, d, q, raw_mask, j, i));
  const uint64_t chunk = (len + 31) / 16 * 16;   // either side of the cut holds the whole row
  std::vector<uint8_t> got;
  for (uint64_t a = 0; a <= len; a++) {
    const uint64_t boundary = chunk, at = boundary - a;   // ob: byte a of the row is output byte `boundary`
    std::vector<uint64_t> ob(k, ~0ull);
    ob[j] = at;
    const pack::View table{ob.data() + j, nullptr, nullptr, nullptr, j, j + 1, at + len};
    for (int side = 0; side < 2; side++) {
      const uint64_t c0 = side ? boundary : 0, c1 = side ? at + len : boundary;
      if (c0 >= c1) continue;
      Checkpoints cps;
      checkpoint_all(src, table, j, j + 1, q, raw_mask, chunk, at + len, &cps);   // (chunks of `chunk` bytes: the cut is the second one's begin)
      const Made m = make_chunk(src, table, j, j + 1, d, q, raw_mask, 0xEE, c0, c1, chunk, &cps, &got);
      if (m.twice || m.left_range || counts.left_range || cps.twice || cps.unwritten || cps.left_range) return -1;
      for (uint64_t p = c0; p < c1; p++) {
        const uint8_t want = p < at ? 0xEE : row_out[p - at];
        if (got[p - c0] != want) return -3;
      }
    }
  }
  return static_cast<long>(len);
}

#ifdef CSV_FORMAT_EXEC_MAIN
#include <stdio.h>
#include <stdlib.h>

#include <string>

namespace {

struct HostColumn {
  std::vector<uint8_t> text;
  std::vector<uint64_t> begins, ends, indices;
  bool with_indices;
};

// a column of n_records records with lengths from `lengths` over an alphabet with the special bytes, packed without slack: the
// sanitizer sees a read behind the text
HostColumn make_column(uint64_t n_records, const std::vector<uint64_t>& lengths, uint64_t k, bool with_indices, int quote_every) {
  static const uint8_t alphabet[] = {'a', 'b', ' ', 0xE9, 0, ',', '"', '\n', '\r', ';', '\''};
  HostColumn h;
  h.with_indices = with_indices;
  for (uint64_t r = 0; r < n_records; r++) {
    const uint64_t len = lengths[rnd(lengths.size())];
    const bool plain = rnd(3) == 0;
    h.begins.push_back(h.text.size());
    for (uint64_t i = 0; i < len; i++) h.text.push_back(plain ? static_cast<uint8_t>('a' + (r + i) % 26) : rnd(quote_every) == 0 ? '"' : alphabet[rnd(sizeof(alphabet))]);
    h.ends.push_back(h.text.size());
  }
  if (with_indices)
    for (uint64_t j = 0; j < k; j++) h.indices.push_back(rnd(n_records));
  return h;
}

std::string want_row(const std::vector<HostColumn>& hs, char d, char q, uint32_t always_mask, uint32_t raw_mask, uint64_t j) {
  std::string row;
  for (size_t c = 0; c < hs.size(); c++) {
    const HostColumn& h = hs[c];
    const uint64_t r = h.with_indices ? h.indices[j] : j;
    const std::string piece(reinterpret_cast<const char*>(h.text.data()) + h.begins[r], h.ends[r] - h.begins[r]);
    bool need = ((always_mask >> c) & 1) != 0 || (hs.size() == 1 && piece.empty());
    for (char b : piece) need |= b == d || b == q || b == '\n' || b == '\r';
    if (c) row += d;
    if (!need) {
      row += piece;
      continue;
    }
    row += q;
    for (char b : piece) {
      row += b;
      if (b == q && !((raw_mask >> c) & 1)) row += q;
    }
    row += q;
  }
  return row;
}

}  // namespace

int main() {
  const std::vector<std::vector<uint64_t>> length_sets = {{0}, {0, 1, 15, 16, 17, 33}, {31, 32, 33}, {3, 8, 200}, {1, 2, 1023, 1024, 1025}, {2, 5000}, {3, 8191, 8192, 20000}};
  const char pairs[3][2] = {{',', '"'}, {';', '\''}, {'\t', '"'}};
  int cases = 0;
  for (int n_cols : {1, 2, 3, 16})
    for (size_t ls = 0; ls < length_sets.size(); ls++)
      for (int layout = 0; layout < 4; layout++) {
        const uint64_t k = 30 + rnd(20);
        const uint64_t lead = layout & 1 ? 5 : 0, gap = layout == 0 ? 0 : layout == 1 ? 1 : layout == 2 ? 3 : 40;
        const char d = pairs[(ls + layout) % 3][0], q = pairs[(ls + layout) % 3][1];
        const uint32_t known = (1u << n_cols) - 1u;
        const uint32_t always_mask = (layout == 2 ? 0x5555u : layout == 3 ? 0xFFFFu : 0u) & known, raw_mask = (layout == 1 ? 0xAAAAu : layout == 3 ? 0x3u : 0u) & known;
        std::vector<HostColumn> hs;
        for (int c = 0; c < n_cols; c++) {
          const bool with_indices = (c + layout) % 2 == 1;
          hs.push_back(make_column(with_indices ? 25 : k, length_sets[ls], k, with_indices, c % 2 ? 4 : 40));
        }
        std::vector<csvf::Column> cols;
        for (const HostColumn& h : hs)
          cols.push_back(csvf::Column{h.text.data(), h.text.size(), h.begins.data(), h.ends.data(), h.begins.size(), h.with_indices ? h.indices.data() : nullptr,
                                      h.with_indices ? h.indices.size() : 0, 0, 0});
        std::string want(lead, '\n');
        std::vector<uint64_t> want_begin, want_end;
        for (uint64_t j = 0; j < k; j++) {
          want_begin.push_back(want.size());
          want += want_row(hs, d, q, always_mask, raw_mask, j);
          want_end.push_back(want.size());
          want += std::string(gap, '\n');
        }
        std::vector<uint64_t> ob(k), oe(k);
        uint64_t summary[13];
        char message[320];
        void* room = nullptr;
        if (posix_memalign(&room, 16, want.size() ? want.size() : 1) != 0) return 1;
        uint8_t* out = static_cast<uint8_t*>(room);
        const uint64_t chunk = layout == 0 ? 64 : layout == 1 ? 4096 : 256;
        const long rc = cfe_format(cols.data(), n_cols, d, q, always_mask, raw_mask, 0, '\n', lead, gap, 16, chunk, out, want.size(), ob.data(), oe.data(), summary,
                                   message);
        const bool same = rc == 0 && summary[0] == want.size() && memcmp(out, want.data(), want.size()) == 0 && ob == want_begin && oe == want_end;
        free(out);
        if (!same) {
          fprintf(stderr, "csv_format_exec: %d columns, lengths %zu, layout %d: rc %ld total %llu want %zu\n", n_cols, ls, layout, rc,
                  static_cast<unsigned long long>(summary[0]), want.size());
          return 1;
        }
        for (uint64_t j = 0; j < k; j += 7) {   // a row at every cut (the work is quadratic in the row: the short ones here)
          if (want_end[j] - want_begin[j] > 400) continue;
          std::vector<uint8_t> row(want_end[j] - want_begin[j] + 1);
          const long len = cfe_row_cuts(cols.data(), n_cols, d, q, always_mask, raw_mask, j, row.data(), row.size());
          if (len != static_cast<long>(want_end[j] - want_begin[j]) || memcmp(row.data(), want.data() + want_begin[j], len) != 0) {
            fprintf(stderr, "csv_format_exec: %d columns, lengths %zu, layout %d, row %llu: cuts %ld\n", n_cols, ls, layout, static_cast<unsigned long long>(j), len);
            return 1;
          }
        }
        cases += static_cast<int>(k);
      }
  printf("csv_format_exec: %d cases\n", cases);
  return 0;
}
#endif
