// nuts_rec_part4.hip — the recording (REC) NUTS kernel instantiations of nuts_part4.hip's layouts.
#define GM_NUTS_REC 1
#include "nuts_part4.hip"
