// C surface of opencv-dlco_amd/csrc/track_rules.hpp for tests/test_track_rules.py: built with g++ into a shared object, no HIP.
#include "../../opencv-dlco_amd/csrc/track_rules.hpp"

namespace tr = track_rules;

extern "C" {

int shim_track_block_nodes() { return tr::kBlockNodes; }
int shim_track_scan_chunk() { return tr::kScanChunk; }
int shim_track_counted() { return tr::kCounted; }

// the edge of match (i, j) between images of na and nb rows that start at nodes a0 and b0: 1 and (u, v), or 0
int shim_track_edge(int32_t a0, int32_t na, int32_t b0, int32_t nb, int32_t i, int32_t j, int32_t *uv)
{
    const tr::Pair pr{0, a0, na, b0, nb};
    return tr::edge_of(pr, i, j, uv, uv + 1) ? 1 : 0;
}

int32_t shim_track_image_of(const int64_t *seg, int32_t n_img, int64_t g) { return tr::image_of(seg, n_img, g); }

int shim_track_moff_ok(const int64_t *moff, int64_t n_pairs) { return tr::moff_ok(moff, n_pairs) ? 1 : 0; }
int shim_track_settings_ok(int32_t min_len, int32_t unique) { return tr::settings_ok(min_len, unique) ? 1 : 0; }

int64_t shim_track_pair_of_match(const int64_t *seg, const int32_t *pairs, int64_t n_pairs, const int64_t *moff, int64_t m)
{
    std::vector<tr::Pair> rec;
    tr::pair_records(seg, pairs, n_pairs, moff, rec);
    return tr::pair_of_match(rec.data(), 0, n_pairs - 1, m);
}

// the hook step over the matches in the order given (null: ascending)
void shim_track_labels(const int64_t *seg, int32_t n_img, const int32_t *pairs, int64_t n_pairs, const int64_t *moff, const int32_t *matches,
                       const uint8_t *keep, const int64_t *order, int32_t *label)
{
    tr::labels_host(seg, n_img, pairs, n_pairs, moff, matches, keep, order, label);
}

int64_t shim_track_build(const int64_t *seg, int32_t n_img, const int32_t *pairs, int64_t n_pairs, const int64_t *moff, const int32_t *matches,
                         const uint8_t *keep, int32_t min_len, int32_t unique, int64_t *toff, int32_t *obs, int32_t *track_of, int32_t *label,
                         int64_t *counts)
{
    return tr::tracks_host(seg, n_img, pairs, n_pairs, moff, matches, keep, min_len, unique, toff, obs, track_of, label, counts);
}

}  // extern "C"
