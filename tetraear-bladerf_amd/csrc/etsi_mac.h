// etsi_mac.h -- what etsi_mac.hip gives the timebase vote's host path (etsi_tdma_vote.hip).
#pragma once
#include "common.h"

// k_mac_walk on the context's stream, as tetra_etsi_mac_groups launches it: the PDU walk of every
// CRC-good block of C rows into npdu / pdus, and own [C][MAXB]: burst b's own-SYNC slot count (an SB
// whose BSCH block is CRC-good with a STATUS 0 record), -1 for none; entries past nburst[c] are not
// written.  Device pointers.
void launch_mac_walk(tetra_ctx *ctx, size_t C, const int32_t *nburst, const int32_t *bursts, const int32_t *nblock,
                     const int32_t *blocks, const uint8_t *type1, int32_t *own, int32_t *npdu, int32_t *pdus);
