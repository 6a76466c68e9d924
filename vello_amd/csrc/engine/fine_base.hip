// fine for frames over a base image (vello_hip_set_base_image): fine.hip compiled a third time as k_fine_base, whose pixels start from
// the lane's own words of the image instead of the base colour, and whose final store is held to the frame's rectangle (the whole
// target without a damage rectangle).  A unit of its own so that k_fine and k_fine_damage stay the code they were (fine.hip says why
// at VK_FINE_DAMAGE and VK_FINE_BASE_IMAGE); everything else -- the interpreter, the batches, the slices -- is the same source.
#define VK_FINE_BASE_IMAGE 1
#include "fine.hip"
