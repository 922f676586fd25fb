/* TEST TOOL: a stand-in for a prebuilt libhs consumer (the reference's shim is one).  Built as a shared object linked
 * against SOME object whose SONAME is libhs.so.5 (tests/test_abi.py links it against the oracle's), with no RPATH or
 * RUNPATH, and importing exactly the libhs symbols tests/golden/reference_shim_abi.json records for the shim.  Loaded after
 * hypergrep_amd/lib/libhs.so.5 has been loaded by path, its DT_NEEDED entry must bind to that already-loaded object.
 *
 *   consumer_compile(exprs, flags, ids, n)      hs_compile_multi's return code (the compile error record is freed)
 *   consumer_scan(expr, data, len, &alloc_rc)   reports of one hs_scan over data, or -1 when hs_alloc_scratch failed
 */
#include <stddef.h>

#include "hypergrep_amd.h"

#define HS_MODE_BLOCK 1

int consumer_compile(const char *const *exprs, const unsigned int *flags, const unsigned int *ids, unsigned int n) {
  hs_database_t *db = NULL;
  hs_compile_error_t *err = NULL;
  int rc = hs_compile_multi(exprs, flags, ids, n, HS_MODE_BLOCK, NULL, &db, &err);
  hs_free_compile_error(err);
  hs_free_database(db);
  return rc;
}

static int on_match(unsigned int id, unsigned long long from, unsigned long long to, unsigned int flags, void *ctx) {
  (void)id;
  (void)from;
  (void)to;
  (void)flags;
  ++*(int *)ctx;
  return 0;
}

int consumer_scan(const char *expr, const char *data, unsigned int len, int *alloc_rc) {
  const char *exprs[1] = {expr};
  const unsigned int flags[1] = {14}; /* DOTALL | MULTILINE | SINGLEMATCH */
  const unsigned int ids[1] = {0};
  hs_database_t *db = NULL;
  hs_compile_error_t *err = NULL;
  hs_scratch_t *scratch = NULL;
  int reports = 0;
  if (hs_compile_multi(exprs, flags, ids, 1, HS_MODE_BLOCK, NULL, &db, &err) != 0) {
    hs_free_compile_error(err);
    return -2;
  }
  *alloc_rc = hs_alloc_scratch(db, &scratch);
  if (*alloc_rc != 0) {
    hs_free_scratch(NULL);
    hs_free_database(db);
    return -1;
  }
  if (hs_scan(db, data, len, 0, scratch, on_match, &reports) != 0) reports = -3;
  hs_free_scratch(scratch);
  hs_free_database(db);
  return reports;
}
