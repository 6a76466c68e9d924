# The library's sources, listed once: the product build (Makefile), the SIMT-emulator build (tests/simt_emu/Makefile) and
# vello_amd._lib.kernel_sources_hash() all read these two lists.  KERNELS are engine/<name>.hip, HOST are host/<name>.cpp.
KERNELS = scan flatten draw clip binning path coarse coarse_damage fine fine_damage fine_base estimate scene_ops pick pick_rect context frames scenes atlas seams
HOST = kurbo encoding resolver scene renderer host_capi
