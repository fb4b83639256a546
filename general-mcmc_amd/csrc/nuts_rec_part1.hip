// nuts_rec_part1.hip — the recording (REC) NUTS kernel instantiations of nuts_part1.hip's layouts.
#define GM_NUTS_REC 1
#include "nuts_part1.hip"
