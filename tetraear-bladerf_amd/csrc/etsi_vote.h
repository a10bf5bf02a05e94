// etsi_vote.h -- what etsi_vote.hip gives the lower MAC's host path (etsi_lmac.hip, lmac_etsi).
#pragma once
#include "common.h"

constexpr size_t VOTE_MAXG = 32;   // rows per group the vote takes (its ballot list is fixed-size)

// k_cell_vote_groups in place of k_cell_acquire / k_cell_acquire_groups, on the context's stream after
// the BSCH pass: NG groups of G <= VOTE_MAXG rows of row_bits soft bytes each, a burst's start bit
// counted from row bit `origin`.  Device pointers; ngood and agree may be null.
void launch_cell_vote(tetra_ctx *ctx, size_t NG, size_t G, const int8_t *softbits, size_t row_bits, int origin,
                      const int32_t *nburst, const int32_t *bursts, const int32_t *blocks, const uint8_t *type1,
                      uint32_t *cell_init, int32_t *score, int32_t cap, int32_t *ngood, int32_t *agree,
                      uint32_t *tab_init, uint8_t *cell_scr);
