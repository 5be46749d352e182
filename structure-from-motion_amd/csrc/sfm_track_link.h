// sfm_track_link.h — the one body behind sfm_link_tracks, sfm_link_tracks_dev and sfm_link_tracks_views (sfm_track_link.hip):
// checked host arrays and device pointers in, everything enqueued on a stream.
#pragma once

#include <vector>

#include "sfm_common.h"

namespace sfm {

struct LinkProblem {
  int V = 0, P = 0, min_len = 2, group = 0, scan = 0;
  const int* key_ptr = nullptr;             // host [V + 1], checked
  const int* pair_views = nullptr;          // host [P][2], checked
  const int64_t* pair_ptr = nullptr;        // host [P + 1], checked
  // the matches, on the device: (a, b) arrays, or one table row per pair (a = the entry's position, b = its value, a match
  // iff b > 0: quirk Q3)
  const int* d_a = nullptr;
  const int* d_b = nullptr;
  const int* const* rows = nullptr;         // host [P] device pointers, or null
  const unsigned char* d_mask = nullptr;    // [M] or null
  // outputs, on the device, each may be null
  int* d_key_track = nullptr;               // [K]
  int* d_pt_ptr = nullptr;                  // [K / 2 + 2]
  int* d_cam_idx = nullptr;                 // [K]
  int* d_key_idx = nullptr;                 // [K]
  int64_t* d_summary = nullptr;             // [8]
  int* d_label = nullptr;                   // [K]
  // the store form: per view the normalised coordinates to gather (host [V] device pointers), and where they go
  const double* const* view_nu = nullptr;
  const double* const* view_nv = nullptr;
  double* d_u = nullptr;                    // [K]
  double* d_v = nullptr;
};

// The argument rules of the rule's refusals that need no match: SFM_E_SHAPE and sfm_last_error, or SFM_OK.
int track_link_check(const char* who, int V, const int* key_ptr, int P, const int* pair_views, const int64_t* pair_ptr, int min_len,
                     int group, int scan);
// Runs the whole chain on s and waits for it; n_tracks / n_obs (may be null) are the two counts the host reads at the end.
// SFM_E_SHAPE with every output untouched when the verify kernel finds a key index out of its view's range.
int track_link_run(const char* who, const LinkProblem& p, int* n_tracks, int64_t* n_obs, hipStream_t s);

}  // namespace sfm
