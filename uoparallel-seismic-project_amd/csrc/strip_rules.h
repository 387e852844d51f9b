// strip_rules.h - decisions of the STRIP driver that need nothing but their arguments (no device, no context): kept
// apart so that a plain C++ program can exercise them (tests/host/strip_rules_main.cpp).
#pragma once

namespace ttsweep {

// The one-launch STRIP solve stores every improved cell into the padded volume AND into the caller's box
// (StartDesc::U).  That keeps the two equal only if they are equal when the solve is launched:
//   fresh boxes (init):  the batched initialisation has filled both (a start initialised by a launch of its own has
//                        only its padded volume filled);
//   boxes with values:   the padded volumes have just been packed from the caller's boxes.
// Every start needs a box on the device.  And the second store has to be cheap: it is kept to the layouts whose lane
// axis is the caller's stride-1 axis z, where the 64 lanes of a store hit consecutive floats of the box (the headline
// grid).  In the other layouts every lane writes a line of its own, write-through, and that costs more than the
// copy it saves (818-FS, 512 x 512 x 256 x 8 starts, lanes along x: 259 -> 267 ms): they keep the copy.
inline bool user_boxes_in_step(bool strip, bool lanes_along_z, bool init, bool batched_init, float *const *tt_dev,
                               int nstart)
{
    if (!strip || !lanes_along_z || !tt_dev || nstart <= 0) return false;
    if (init && !batched_init) return false;
    for (int s = 0; s < nstart; s++)
        if (!tt_dev[s]) return false;
    return true;
}

// The copy from the padded volumes back to the caller's boxes may be left out only when the boxes were in step at the
// launch, the one-launch solve itself ran to rest, and no other driver stored anything after it.  (Copying when it is
// not needed is always correct; not copying when it is needed is not.)
inline bool unpack_can_be_skipped(bool in_step, bool one_launch_at_rest, bool fell_back)
{
    return in_step && one_launch_at_rest && !fell_back;
}

} // namespace ttsweep
