// What the tracker's update entries (csrc/track.hip, track_motion.hip, track_interval.hip, track_cut.hip) share: the arguments of a call as
// one record, the one check of them, the one walk over a call's frames, and the launches the walk issues (a kernel is launched from the
// translation unit that defines it).  Each of the eight entries fills a TrackCall, checks it and walks it.
#pragma once
#include "common.h"

namespace frcnn {

// What an entry has beyond frcnn_track_update: nothing; the motion state, the source frames, ``radius`` and ``interval``; those and the cut step
enum TrackForm { TRACK_PLAIN, TRACK_MOTION, TRACK_CUT };

// The arguments of frcnn_track_update_cut_weak, the widest entry, by name.  ``form`` says which groups the entry HAS -- a null pointer in a
// group it has is refused, not read as "absent" -- and a group it has not stays zero and is never read:
//   TRACK_PLAIN    no motion_state, frames_u8, frame_stride, radius (interval is 1): plain tracking, one launch over all frames;
//   TRACK_MOTION   no pct, workspace, cuts: no cut step.  frcnn_track_update_motion is this form with interval 1, an ordinary value;
//   strong null    the Tracking rule; else the Weak rule's threshold (frcnn_hip_track_weak.h), a HOST value read before the call returns.
struct TrackCall {
    TrackForm form;
    int32_t* state; int capacity;
    uint8_t* motion_state; const uint8_t* frames_u8; long long frame_stride;
    const int32_t* det_packed; long long det_stride; int frames; const int32_t* n_frames; int max_rows;
    const uint8_t* tracked; int num_classes;
    int thr, hold, grow, radius, interval, h, w;
    const float* strong;
    int32_t* out; long long out_stride;
    int pct; int32_t* workspace; int32_t* cuts;
};

// FRCNN_OK, or FRCNN_E_ARG with the message set under the name ``who``: everything the family refuses, in one order for every form
// (interval; the tracking arguments; the motion ones; pct; workspace and cuts; strong).  Launches nothing.
int track_call_check(const char* who, const TrackCall& c);

// A checked call's launches.  TRACK_PLAIN: the tracker kernel once, over all frames.  Else per frame f: k_cut_apply (TRACK_CUT), the motion
// search, then the tracker kernel on frame f's own buffers when f % interval == 0 and k_interval_between otherwise; the keep kernel
// follows behind the last frame.  (The cut form's clear, signatures and decide launches are track_cut.hip's, in front of the walk.)
int track_walk(const char* who, const TrackCall& c, hipStream_t stream);

// track.hip: steps 1-4 over ``frames`` frames from frame ``first`` of the call on, in one launch; ``det`` and ``out`` are frame ``first``'s
void track_launch(const TrackCall& c, int first, int frames, const int32_t* det, int32_t* out, hipStream_t stream);

// track_motion.hip: step 0 of frame ``f``, one workgroup per slot of the state; behind a call's last frame, frame nf - 1 and the header
// into the motion state
void motion_search_launch(const TrackCall& c, int f, hipStream_t stream);
void motion_keep_launch(const TrackCall& c, hipStream_t stream);

// track_interval.hip: between frame ``f``: its tracked buffer ``out`` from the slots as they stand; the frame counts
void interval_between_launch(const TrackCall& c, int f, int32_t* out, hipStream_t stream);

// track_cut.hip: step C of frame ``f``: the slots freed where cuts[f] is set
void cut_apply_launch(const TrackCall& c, int f, hipStream_t stream);

}  // namespace frcnn
