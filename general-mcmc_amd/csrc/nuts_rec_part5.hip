// nuts_rec_part5.hip — the recording (REC) NUTS kernel instantiations of nuts_part5.hip's layouts.
#define GM_NUTS_REC 1
#include "nuts_part5.hip"
