"""No-GPU check of hnswgpu_pcaf_add / _remove / _update: the entry points exist and are bound."""
import subprocess

import pytest


@pytest.mark.parametrize("name,sig", [
    ("hnswgpu_pcaf_add", ["p", "p", "i64"]),            # idx rows m
    ("hnswgpu_pcaf_remove", ["p", "p", "i64", "p"]),    # idx rows m n_after
    ("hnswgpu_pcaf_update", ["p", "p", "p", "i64"]),    # idx ids rows m
])
def test_pcaf_mutation_symbol_is_exported_and_bound(native_lib, name, sig):
    syms = subprocess.run(["nm", "-D", native_lib.SO], check=True, capture_output=True, text=True).stdout
    assert any(line.split()[-1] == name and " T " in line for line in syms.splitlines()), "nm -D: no %s" % name
    assert name in native_lib.EXPORTS
    assert native_lib._SIGS[name] == sig
    assert getattr(native_lib.lib(), name).argtypes is not None
    assert native_lib.lib().hnswgpu_version() == 104    # the new symbols are additive
