// aeth_chan_fold.h -- the analysis bank's object and its fold launch (aeth_chan.hip), shared with the synthesis bank
// (aeth_synth.hip): with hop == M the overlap-add is the fold of the row-reversed prototype, so it runs these kernels.
#pragma once
#include "aeth_internal.h"

struct aeth_chan {
    aeth_ctx *ctx = nullptr;
    size_t M = 0, L = 0, P = 0, D = 0;
    int phase = 0;
    bool ring = false;           // hop == M and P <= 8
    size_t tile = 0;
    float *w_dev = nullptr;
    aeth_fft *fft = nullptr;
    float2 *scratch = nullptr;   // the folded frames of exec / exec_levels, grown on demand
    size_t scratch_elems = 0;
};

namespace aeth {

// ring and tile from M, P and D
void chan_geometry(aeth_chan *c);
// workgroups of a launch over F frames, at most
size_t chan_grid_bound(const aeth_chan *c, size_t F);
// the fold of F frames into out on the context's stream; every argument has been checked
int chan_launch_fold(const aeth_chan *c, const aeth_cf32 *hist, const aeth_cf32 *in, size_t F, uint64_t first_frame, float2 *out);

}  // namespace aeth
