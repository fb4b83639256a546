// nuts_rec_part0.hip — the recording (REC) NUTS kernel instantiations of nuts_part0.hip's layouts.
#define GM_NUTS_REC 1
#include "nuts_part0.hip"
