// nuts_wide_rec.hip — the recording (REC) NUTS kernel instantiations of nuts_wide.hip's layouts.
#define GM_NUTS_REC 1
#include "nuts_wide.hip"
