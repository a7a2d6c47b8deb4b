// Host build of csrc/entryrec.h for tests/test_pair_rows_cpu.py (test infrastructure, g++ only).
#include "../humangaussian_amd/csrc/entryrec.h"
extern "C" void hgs_rec_tag_host(int n_, const uint32_t* mask, const uint32_t* k, const uint32_t* n, const uint32_t* chunk_rows,
                                 uint32_t* out) {
  for (int i = 0; i < n_; ++i) out[i] = hgs_rec_tag(mask[i], k[i], n[i], chunk_rows[i] != 0u);
}
// out[4 i ..]: mask, position in the chunk, records of the chunk, chunk-rows bit
extern "C" void hgs_tag_fields_host(int n_, const uint32_t* tag, uint32_t* out) {
  for (int i = 0; i < n_; ++i) {
    out[4 * i] = hgs_tag_mask(tag[i]);
    out[4 * i + 1] = hgs_tag_pos(tag[i]);
    out[4 * i + 2] = hgs_tag_count(tag[i]);
    out[4 * i + 3] = hgs_tag_chunk_rows(tag[i]) ? 1u : 0u;
  }
}
extern "C" void hgs_entpair_x_host(int n_, const uint32_t* entry, const uint32_t* pairs, uint32_t* out) {
  for (int i = 0; i < n_; ++i) out[i] = hgs_entpair_x(entry[i], pairs[i]);
}
extern "C" void hgs_entpair_entry_host(int n_, const uint32_t* x, uint32_t* out) {
  for (int i = 0; i < n_; ++i) out[i] = hgs_entpair_entry(x[i]);
}
extern "C" void hgs_entpair_pairs_host(int n_, const uint32_t* x, uint32_t* out) {
  for (int i = 0; i < n_; ++i) out[i] = hgs_entpair_pairs(x[i]);
}
