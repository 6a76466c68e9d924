// fine for frames with a damage rectangle (vello_hip_set_damage_rect): fine.hip compiled once more as k_fine_damage, whose final store
// is held to the rectangle.  A unit of its own so that k_fine, the kernels of whole frames, stays the code it was (fine.hip says
// why at VK_FINE_DAMAGE); everything else -- the interpreter, the batches, the slices -- is the same source.
#define VK_FINE_DAMAGE 1
#include "fine.hip"
