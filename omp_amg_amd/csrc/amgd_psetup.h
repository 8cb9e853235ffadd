/*
 * amgd_psetup.h -- the partitioned multi-GPU setup (amgd_psetup.c) as seen by the entry
 * point amgd_setup_device (amgd_setup.c), which runs it when the library communicator is
 * in partitioned mode.  Its counters (amgd_part_stats) are declared in amgd.h.
 */
#ifndef AMGD_PSETUP_H
#define AMGD_PSETUP_H
#include "amgd_drv.h"

/* this rank's COO entries (global indices, any rows; every rank's together are the
   matrix, duplicates summed in rank order) -> this rank's row blocks in h (part = 1) */
int amgd_psetup_body(uint64_t nz, const uint32_t *dAi, const uint32_t *dAj, const double *dAv,
                     amgd_hier *h, amgd_stats *st);
#endif
