// seqhead_check.cpp — stand-alone host check of the index arithmetic of the sequence/head exchange copies
// (ring-flash-attention_amd/csrc/rfa_seqhead_index.h: the ONE function the gfx950 kernel uses as well).  No GPU, no HIP:
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -I ring-flash-attention_amd/csrc tests/native/seqhead_check.cpp
// For every op x layout over U in {1,2,3,8}, B in {1,2}, S in {1,2,5,64} (even S for zigzag), P in {1,2,3}, Hs in {1,3},
// D in {8,72}, with a padded strided side, it enumerates EVERY chunk exactly as the launch does and checks that
//   * the source and the destination offsets (all 8 elements) lie inside their buffers,
//   * the map is a bijection between the slot buffer and the elements of the strided view (nothing is written twice, every
//     element of the view is reached, padding between rows is never touched),
//   * the copy it describes, run on real buffers, is undone by the inverse op,
//   * the merged row agrees with the table of the layouts written out independently below.
// Exit status 0 and "seqhead_check: N configurations ok" on success; the first failure is printed and the status is 1.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rfa_seqhead_index.h"

using namespace rfa;

static int fail(const char* what, int op, int layout, int U, int B, int S, int P, int Hs, int D) {
  std::printf("seqhead_check: FAILED: %s (op %d layout %d U %d B %d S %d P %d Hs %d D %d)\n", what, op, layout, U, B, S, P, Hs, D);
  return 1;
}

// the table of the layouts, written the slow way: walk the U ranks' rows in the order the wrapped schedule wants them
static std::vector<int> merged_rows_by_table(int layout, int U, int S) {
  std::vector<int> m(U * S, -1);           // m[j*S + i]
  int next = 0;
  if (layout == kSeqHeadContiguous) {
    for (int j = 0; j < U; ++j) for (int i = 0; i < S; ++i) m[j * S + i] = next++;
  } else if (layout == kSeqHeadStripe) {
    for (int i = 0; i < S; ++i) for (int j = 0; j < U; ++j) m[j * S + i] = next++;
  } else {
    const int C = S / 2;                   // fronts of ranks 0 .. U-1, then backs of ranks U-1 .. 0
    for (int j = 0; j < U; ++j) for (int i = 0; i < C; ++i) m[j * S + i] = next++;
    for (int j = U - 1; j >= 0; --j) for (int i = C; i < S; ++i) m[j * S + i] = next++;
  }
  return m;
}

static int check(int op, int layout, int U, int B, int S, int P, int Hs, int D) {
  const bool local = op == kSeqHeadPack || op == kSeqHeadSlotsToHeads;
  const int rows = local ? S : U * S, heads = local ? U * Hs : Hs;
  // a padded strided side: 8 spare elements after every head, 16 after every part, 24 after every row, 32 after a batch
  SeqHeadTensor t{};
  t.head = D + 8;
  t.part = (int64_t)heads * t.head + 16;
  t.row = (int64_t)P * t.part + 24;
  t.batch = (int64_t)rows * t.row + 32;
  t.slot_base = 40;                        // (as if a first tensor of 40 elements shared the slots)
  t.P = P; t.Hs = Hs; t.rowchunks = P * Hs * (D / 8);
  t.nchunks = (uint32_t)U * B * S * t.rowchunks;
  SeqHeadGeom g{};
  g.op = op; g.layout = layout; g.U = U; g.B = B; g.S = S; g.D8 = D / 8;
  const int64_t part_elems = (int64_t)B * S * t.rowchunks * 8;
  g.slot_stride = t.slot_base + part_elems + 16;     // (... and a third one of 16 behind)
  const int64_t nslot = (int64_t)U * g.slot_stride, nstr = (int64_t)B * t.batch;
  std::vector<int32_t> slot_hit(nslot, 0), str_hit(nstr, 0);
  std::vector<uint16_t> slots(nslot, 0), strided(nstr, 0), back(seqhead_from_slots(op) ? nslot : nstr, 0);
  // fill the source with a pattern that names the position
  std::vector<uint16_t>& src = seqhead_from_slots(op) ? slots : strided;
  for (size_t x = 0; x < src.size(); ++x) src[x] = (uint16_t)(x * 40503u + 17u);
  const std::vector<int> table = merged_rows_by_table(layout, U, S);
  for (uint32_t c = 0; c < t.nchunks; ++c) {
    int64_t so, to;
    seqhead_chunk(g, t, c, &so, &to);
    if (so < 0 || so + 8 > nslot) return fail("slot offset out of bounds", op, layout, U, B, S, P, Hs, D);
    if (to < 0 || to + 8 > nstr) return fail("strided offset out of bounds", op, layout, U, B, S, P, Hs, D);
    if ((so & 7) || (to & 7)) return fail("offset not a multiple of 16 bytes", op, layout, U, B, S, P, Hs, D);
    for (int e = 0; e < 8; ++e) {
      if (slot_hit[so + e]++ || str_hit[to + e]++) return fail("an element is visited twice", op, layout, U, B, S, P, Hs, D);
      if (seqhead_from_slots(op)) strided[to + e] = slots[so + e];
      else slots[so + e] = strided[to + e];
    }
  }
  // the slot side: exactly this tensor's part of every slot
  for (int64_t x = 0; x < nslot; ++x) {
    const int64_t in = x % g.slot_stride;
    const int want = in >= t.slot_base && in < t.slot_base + part_elems;
    if (slot_hit[x] != want) return fail("slot side is not covered exactly", op, layout, U, B, S, P, Hs, D);
  }
  // the strided side: exactly the elements of the (B, rows, P, heads, D) view, no padding
  for (int64_t x = 0; x < nstr; ++x) {
    int64_t r = x;
    const int64_t b = r / t.batch; r %= t.batch;
    const int64_t row = r / t.row; r %= t.row;
    const int64_t p = r / t.part; r %= t.part;
    const int64_t h = r / t.head; r %= t.head;
    const int want = b < B && row < rows && p < P && h < heads && r < D;
    if (str_hit[x] != want) return fail("strided side is not covered exactly", op, layout, U, B, S, P, Hs, D);
  }
  // the merged row against the table
  if (!local)
    for (int j = 0; j < U; ++j)
      for (int i = 0; i < S; ++i)
        if ((int)seqhead_merged_row(layout, U, S, j, i) != table[j * S + i])
          return fail("merged row differs from the table", op, layout, U, B, S, P, Hs, D);
  // the inverse op undoes it
  SeqHeadGeom gi = g;
  gi.op = op == kSeqHeadPack ? kSeqHeadSlotsToHeads : op == kSeqHeadSlotsToHeads ? kSeqHeadPack
        : op == kSeqHeadUnpack ? kSeqHeadMergedToSlots : kSeqHeadUnpack;
  const std::vector<uint16_t>& mid = seqhead_from_slots(op) ? strided : slots;
  for (uint32_t c = 0; c < t.nchunks; ++c) {
    int64_t so, to;
    seqhead_chunk(gi, t, c, &so, &to);
    for (int e = 0; e < 8; ++e) {
      if (seqhead_from_slots(gi.op)) back[to + e] = mid[so + e];
      else back[so + e] = mid[to + e];
    }
  }
  const std::vector<int32_t>& hit = seqhead_from_slots(op) ? slot_hit : str_hit;
  for (size_t x = 0; x < back.size(); ++x)
    if (hit[x] && back[x] != src[x]) return fail("the inverse op does not undo it", op, layout, U, B, S, P, Hs, D);
  return 0;
}

int main() {
  const int Us[] = {1, 2, 3, 8}, Bs[] = {1, 2}, Ss[] = {1, 2, 5, 64}, Ps[] = {1, 2, 3}, Hss[] = {1, 3}, Ds[] = {8, 72};
  long n = 0;
  for (int op = 0; op < 4; ++op)
    for (int layout = 0; layout < 3; ++layout)
      for (int U : Us) for (int B : Bs) for (int S : Ss) for (int P : Ps) for (int Hs : Hss) for (int D : Ds) {
        if (layout == kSeqHeadZigzag && (S & 1)) continue;
        if (check(op, layout, U, B, S, P, Hs, D)) return 1;
        ++n;
      }
  std::printf("seqhead_check: %ld configurations ok\n", n);
  return 0;
}
