// bitmapperbs_amd/csrc/bmbs_rowpitch.h -- the pitch rule of the lane's packed read rows (k_rows.hip), on its own so that a host program
// can compile the very lines the kernels and the launch code use (tests/test_row_pitch.py defines __host__ / __device__ away).
// A row is W = ceil(L / 32) words of bases and M = ceil(L / 64) words of not-ACGT marks, rows pack_words(L) words apart: W + M rounded
// up to whole 64-byte lines (8 words) -- 100 and 150 bases -> 8, 250 -> 16, 500 -> 24.  There is no spare word behind a row.
#pragma once
__host__ __device__ inline int pack_base_words(int L) { return (L + 31) / 32; }
__host__ __device__ inline int pack_words(int L) { return ((L + 31) / 32 + (L + 63) / 64 + 7) & ~7; }
