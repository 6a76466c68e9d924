// coarse for frames with a damage rectangle (vello_hip_set_damage_rect): coarse.hip compiled once more as k_coarse_damage, which takes
// the frame's tile window.  A unit of its own so that k_coarse, the kernel of whole frames, stays the code it was (coarse.hip says so
// at VK_COARSE_DAMAGE); k_coarse_prep is not part of it: it runs whole for every frame.
#define VK_COARSE_DAMAGE 1
#include "coarse.hip"
