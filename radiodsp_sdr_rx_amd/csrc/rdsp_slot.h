/*
 * rdsp_slot.h -- the double-buffering of a table that kernels read while the host replaces it between calls (rdsp_chain_t's
 * per-group filter masks and rotated branch spectra), as a state machine with no HIP in it: rdsp_chain_int.h's GroupSlot owns
 * the resources and follows it, the host program of the tests (tests/host/host_slot_check.cpp) walks it.
 *
 * The table has two device halves and two pinned host images.  The device record points at the half `live`.  A fill writes
 * the next image and uploads it into the other half -- or again into the half that already holds newer contents not yet
 * switched in -- and the record, rewritten in stream order, switches over.  Images alternate, so the one a fill writes was
 * last read by the upload two fills back: the one upload whose event the host has to wait for before it overwrites the image.
 */
#ifndef RDSP_SLOT_H
#define RDSP_SLOT_H

namespace rdsp_slot {

struct Fill {
  int image, target; /* the pinned image to write, the device half to upload it into */
};

struct Slot {
  int live = 0;       /* the half the device record points to (as queued) */
  int pending = -1;   /* the half holding newer contents that are not yet switched in; -1: none */
  int next_image = 0; /* the image the next fill uses */
  int last_image = 0; /* the image the last fill used: its upload is the one a switch has to be ordered behind */

  Fill fill() {
    const Fill f = {next_image, pending >= 0 ? pending : 1 - live};
    last_image = f.image;
    next_image = f.image ^ 1;
    pending = f.target;
    return f;
  }
  void switch_over() {
    if (pending >= 0) live = pending;
    pending = -1;
  }
  /* the halves' contents are gone and nothing is queued; the images go on alternating */
  void reset() { live = 0, pending = -1; }
};

}  // namespace rdsp_slot

#endif
