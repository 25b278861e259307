"""KV-cache slots of generate_many() for standard_mha, the host side: the capacity and rotary-table arithmetic as pure
functions, and the opt-in switch (off by default, read from APERTIS_MHA_SLOTS at import)."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("lens, budgets, cap", [
    ([1, 2, 5, 9, 17, 33, 40], [30] * 7, 69),             # 40 + 30 - 1
    ([1, 2, 5, 9, 17, 33, 40], [1, 0, 7, 30, 30, 16, 3], 48),     # 33 + 16 - 1 against 17 + 30 - 1 = 46 and 40 + 3 - 1 = 42
    ([7], [1], 7),                                        # one token: the prefill's rows and no step
    ([7], [2], 8),                                        # one step, appending row 7
    ([1], [0], 1),                                        # nothing to generate: at least one row
    ([1], [1], 1),
    ([], [], 1),
    ([200, 1920], [128, 128], 2047),
])
def test_slot_capacity(lens, budgets, cap):
    from apertis_llm_amd.serving import mha_slot_capacity
    assert mha_slot_capacity(lens, budgets) == cap


@pytest.mark.parametrize("lens, budgets, max_pos, bad", [
    ([40, 40], [89, 90], 128, 1),                         # 40 + 89 - 1 = 128 fits, 129 does not
    ([128], [1], 128, None),                              # the prefill alone fills the table
    ([129], [1], 128, 0),
    ([128], [2], 128, 0),                                 # its one step would sit at position 128
    ([128], [0], 128, None),
    ([129], [0], 128, None),                              # 129 + 0 - 1 = 128: nothing runs, nothing to refuse
    ([1920, 200], [128, 256], 2048, None),
    ([1920, 200], [130, 256], 2048, 0),
    ([], [], 128, None),
])
def test_rotary_table_bound(lens, budgets, max_pos, bad):
    from apertis_llm_amd.serving import mha_slot_overrun
    assert mha_slot_overrun(lens, budgets, max_pos) == bad


def test_a_prompt_that_fits_the_table_fits_the_slot():
    from apertis_llm_amd.serving import mha_slot_capacity, mha_slot_overrun
    lens, budgets = [3, 60, 127, 128], [126, 69, 2, 1]
    assert mha_slot_overrun(lens, budgets, 128) is None and mha_slot_capacity(lens, budgets) == 128


def _switch(env_value):
    env = {k: v for k, v in os.environ.items() if k != "APERTIS_MHA_SLOTS"}
    if env_value is not None:
        env["APERTIS_MHA_SLOTS"] = env_value
    code = ("from apertis_llm_amd import ops; from apertis_llm_amd.ops import attention; "
            "assert ops.ATTN_SLOTS is attention.ATTN_SLOTS; print(ops.ATTN_SLOTS)")
    return subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, check=True).stdout.strip()


def test_switch_is_off_by_default_and_reads_its_environment_variable():
    assert _switch(None) == "False"
    assert _switch("1") == "True"


def test_switch_is_forwarded_by_the_ops_package(monkeypatch):
    from apertis_llm_amd import ops
    from apertis_llm_amd.ops import attention
    monkeypatch.setattr(ops, "ATTN_SLOTS", True)
    assert attention.ATTN_SLOTS is True
    monkeypatch.setattr(ops, "ATTN_SLOTS", False)
    assert attention.ATTN_SLOTS is False
