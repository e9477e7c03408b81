/*
 * prune_unit.hip -- the one translation unit of the selection, resident, level and random-pruning
 * kernels.  Each family has its own file, and each of them compiles on its own (the labs of
 * tools/mb include the ones they need), but the library compiles them together: the machine code
 * of k_resident and of select_body's callers depends on which kernels share a unit (the inline HIP
 * helpers they call are optimized over all their callers), and any change of k_resident's code,
 * even one of register numbering, has moved its time by about 1 % (profiles/refactor_split_ab.txt).
 */
#include "select.inc"    /* window, collect, fused selection, mask-select, min-weight pruning */
#include "resident.inc"  /* k_resident and its host-side knobs */
#include "levels.inc"    /* per-level filter bank, copy-threshold, synth, count-small */
#include "randprune.inc" /* random pruning */
