/* prints sizeof of every struct of include/akmi.h that athenak_amd/capi.py mirrors (tests/test_capi_symbols.py) */
#include <stdio.h>

#include "akmi.h"

#define SIZE_OF(t) printf(#t " %zu\n", sizeof(t))

int main(void) {
  SIZE_OF(akmi_pack);
  SIZE_OF(akmi_smr);
  SIZE_OF(akmi_rng_state);
  SIZE_OF(akmi_srcterms);
  SIZE_OF(akmi_pdf_axis);
  SIZE_OF(akmi_coarsen_var);
  SIZE_OF(akmi_mg_plan);
  return 0;
}
