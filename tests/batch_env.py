"""The batch size of a device text path, set for the calls inside a `with`: the tests of the validPairs, Juicer and significances
paths put batch edges inside small files with it (csrc/fhx_textupload.hpp reads the variable when a call opens its file)."""
import contextlib
import os


@contextlib.contextmanager
def batch_bytes(var, n):
    """FHX_VP_BATCH_BYTES, FHX_JC_BATCH_BYTES or FHX_MS_BATCH_BYTES (`var`) = n for the calls inside (None: the default)"""
    if n is None:
        yield
        return
    os.environ[var] = str(n)
    try:
        yield
    finally:
        del os.environ[var]
