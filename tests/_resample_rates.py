"""Test infrastructure: the sampling-rate pairs tests/test_gpu_resample_mfma.py runs ``resample_mfma_kernel`` at, with what each one is there
for.  tests/test_resample_tables.py holds the list to that purpose on the CPU (every hop-tile instance, both parities of the tap loop's
trip count, fewer / as many / more phase tiles than the workgroup has waves), so that an edit of the list shows what it gives up.

geometry (lhotse_amd/csrc/resample_tables.hpp): orig : new reduced, kw = 2 width + orig taps, kwp = kw rounded up to 16, HT = hop tiles
of a workgroup (the template instance), phase tiles = ceil(new / 16) dealt to 4 waves."""

# the ratios the library routes to the matrix-core kernel by itself (many phases, odd hop)
ROUTED = [(44100, 16000), (22050, 16000), (11025, 16000), (44100, 24000)]  # 441:160, 441:320, 441:640 (HT 2), 147:80 (HT 4, 5 phase tiles)
ROUTED_IDS = ["441:160", "441:320", "441:640", "147:80"]
# an even hop, which the routing rule leaves to the generic kernel: HIPFEAT_RESAMPLE_MFMA=1 puts it on the matrix cores
EVEN_HOP = (16000, 44100)  # 160:441 (HT 4, 28 phase tiles)
# the only instance with ONE hop tile per workgroup: orig of ~520 ... 1050; an even hop as well, so it is forced like EVEN_HOP
ONE_HOP_TILE = (16000, 11025)  # 640:441: kw 658, kwp 672 = 42 trips, 28 phase tiles of which the last holds 9 phases
# a single phase tile (waves 1-3 of a workgroup have no work) and an odd hop: routed
ONE_PHASE_TILE = (24500, 8000)  # 49:16
# exactly as many phase tiles as waves: routed
FOUR_PHASE_TILES = (22050, 9600)  # 147:64
EXTRA = [ONE_HOP_TILE, ONE_PHASE_TILE, FOUR_PHASE_TILES]
EXTRA_IDS = ["640:441", "49:16", "147:64"]
ALL = ROUTED + [EVEN_HOP] + EXTRA
