/* Stand-alone caller of the C++ host for tests/test_host_unwind.py: on a machine without a device every akmi_sim_create
 * fails at its first device allocation, after the Mesh, the MeshBlockPack and the MeshBlock tables have been built.  Linked
 * with host files compiled under AddressSanitizer, LeakSanitizer reports at exit whatever those failed creates left behind. */
#include <stdio.h>
#include <stdlib.h>
#include "../include/akmi.h"

int main(int argc, char **argv) {
  static char deck[1 << 16];
  long long out[1];
  FILE *f = argc > 1 ? fopen(argv[1], "rb") : NULL;
  if (!f) { fprintf(stderr, "usage: %s deck.athinput\n", argv[0]); return 2; }
  deck[fread(deck, 1, sizeof(deck) - 1, f)] = '\0';
  fclose(f);
  for (int i = 0; i < 3; ++i) {
    void *h = akmi_sim_create(deck, NULL);
    if (h) { fprintf(stderr, "akmi_sim_create returned a simulation: is there a device?\n"); return 3; }
    printf("create %d: %s\n", i, akmi_last_error());
  }
  /* the host-only Mesh of the exchange plan (2 ranks): built and destroyed on the success path */
  printf("plan entries: %lld\n", akmi_host_exchange_plan(deck, 0, 2, 5, 1, out, 0));
  return 0;
}
