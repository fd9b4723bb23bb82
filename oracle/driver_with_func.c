/* TEST INFRASTRUCTURE — the harness and the generated problem file as ONE translation unit (oracle/Makefile lib*_forms.so):
 * the forms the generated file emits for batched back-ends (bp_tensor_basis and the factored tables, ilqg_step_part,
 * ilqg_deriv_prepare / ilqg_deriv_part) are static there, so only a file that includes it can call them.  Everything else
 * is the driver build it stands beside: same sources, same flags. */
#define DRV_FUNC_IN_UNIT 1
#include "iLQG_func.c"
#include "driver.c"
