"""The quantising row producers (csrc/rows_q.hip) keep their blocks in registers: no private segment, no spills."""
import pytest

import kernel_meta

KERNELS = [("k_mix_rows_q", (1,)), ("k_mix_rows_q", (2,)), "k_v6_mix2_rows_q", "k_groupnorm_rows_q"]   # (1, 2: FORM_ROWS, FORM_SEGS)


@pytest.mark.skipif(not kernel_meta.have_hipcc(), reason="needs hipcc")
def test_rows_q_kernels_have_no_scratch():
    found = kernel_meta.no_scratch("rows_q.hip", KERNELS)
    print({str(k): (v.vgprs, v.wg) for k, v in found.items()})
