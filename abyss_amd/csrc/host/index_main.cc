// abyss-index -- drop-in for the reference's abyss-index (Map/index.cc): FILE.fai and FILE.fm, byte for byte.  The suffix array
// and the BWT come from the GPU through abg_fm_build / abg_fm_export (include/abyss_amd.h); the files are written by
// map_core.h.  No CPU fallback: without a HIP device --fm and --both fail.
#define ABG_INDEX_MAIN 1
#include "map_main.cc"
