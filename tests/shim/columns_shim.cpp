// Host-only test shim, third of three: prints, as one JSON document, the column-cut schedules that field.h's
// plan_columns() chose for the multipliers of every field -- the same compile-time tables the gfx950 kernels are
// built from.  tests/test_field_columns_host.py recomputes every chain from the modulus alone and compares.
// Test infrastructure only.
#include <stdio.h>
#include "../../kzg_snark_amd/csrc/field.h"
using namespace kzg;

template <int NCOL, int NG>
static void print_plan(const char* name, int terms, int units, int square, const ColumnPlan<NCOL, NG>& plan, bool last) {
  printf("    {\"name\": \"%s\", \"terms\": %d, \"units\": %d, \"square\": %d, \"cuts\": %d, \"fits\": %d, \"carry_max\": %llu, \"cut\": [",
         name, terms, units, square, plan.cuts, plan.fits ? 1 : 0, (unsigned long long)plan.carry_max);
  for (int k = 0; k < NCOL; ++k) {
    printf("%s[", k ? ", " : "");
    for (int g = 0; g < NG; ++g) printf("%s%d", g ? ", " : "", plan.cut[k][g] ? 1 : 0);
    printf("]");
  }
  printf("]}%s\n", last ? "" : ",");
}

template <class F>
static void print_field(const char* name, bool last) {
  printf("  {\"field\": \"%s\", \"L\": %d, \"N\": %d, \"fit\": %d, \"top_limb_bound\": %u, \"p\": [", name, F::L, F::N,
         Field<F>::FIT, TopLimb<F>::declared ? TopLimb<F>::bound : 0u);
  for (int j = 0; j < F::N; ++j) printf("%s%u", j ? ", " : "", F::P[j]);
  printf("], \"plans\": [\n");
  print_plan("mul", 1, 1, 0, Columns<F, 1, 1, false>::plan, false);
  print_plan("sqr", 1, 1, 1, Columns<F, 1, 1, true>::plan, false);
  print_plan("mul2", 2, 1, 0, Columns<F, 2, 1, false>::plan, false);
  print_plan("dot<3>", 3, 1, 0, Columns<F, 3, 1, false>::plan, false);
  print_plan("dot<6>", 6, 1, 0, Columns<F, 6, 1, false>::plan, false);
  print_plan("dot<16>", 16, 1, 0, Columns<F, 16, 1, false>::plan, true);
  printf("  ]}%s\n", last ? "" : ",");
}

int main() {
  printf("[\n");
  print_field<BnFr>("bn254_fr", false);
  print_field<BnFp>("bn254_fp", false);
  print_field<BlsFr>("bls12_381_fr", false);
  print_field<BlsFp>("bls12_381_fp", true);
  printf("]\n");
  return 0;
}
