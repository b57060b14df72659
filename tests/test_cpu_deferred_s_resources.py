"""The kernels of the deferred-s form of the fused STPCG (stpcg.hip: k_cg_pupdate_ds<false | true>, and k_cg_update_ns, the
A-step of its odd iterations) must be resident like the kernels they stand in for: 1024-thread workgroups, TWO per CU --
at most 64 vector registers, no scratch memory, at most 80 scalar registers (the cliff of test_cpu_kernel_resources.py) --
and adding them must leave the registers of k_cg_update and k_cg_pupdate where they were.  Read from the compiler's
resource-usage remarks; no GPU needed."""
import os

import pytest

from test_cpu_kernel_resources import HIPCC, _resource_usage


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_deferred_s_kernels_are_resident_like_the_kernels_they_replace():
    cg = _resource_usage("stpcg.hip")
    # the two forms of the direction kernel: four prefetched streams in the flush form
    for n in ("k_cg_pupdate_ds<false>", "k_cg_pupdate_ds<true>"):
        assert n in cg, sorted(cg)[:8]
        sg, vg, _, scratch = cg[n]
        assert sg <= 80 and vg <= 64 and scratch == 0, (n, sg, vg, scratch)
    # the A-step without the boundary step: every instantiation the single-context solve launches, against its twin
    twins = [("k_cg_update_ns<0, false, %d, mi::NoFold>" % kc, "k_cg_update<0, false, %d, mi::NoFold>" % kc)
             for kc in (3, 4, 6, 9, 18, 24, 31, 39)]
    twins += [("k_cg_update_ns<%d, false, 3, mi::NoFold>" % pre, "k_cg_update<%d, false, 3, mi::NoFold>" % pre)
              for pre in (1, 2, 3)]
    twins += [("k_cg_update_ns_s80<0, false, 16, mi::NoFold>", "k_cg_update_s80<0, false, 16, mi::NoFold>")]
    for ns, full in twins:
        assert ns in cg and full in cg, (ns, full)
        (sg, vg, occ, scratch), (sg0, vg0, occ0, scratch0) = cg[ns], cg[full]
        assert sg <= sg0 and scratch <= scratch0, (ns, cg[ns], cg[full])
        if vg0 <= 64:  # (the rows of 5 ... 8 doubles run one workgroup per CU in either kernel)
            assert sg <= 80 and vg <= 64, (ns, cg[ns])
        else:
            assert occ >= 4 and occ0 >= 4 and (occ >= 8) == (occ0 >= 8), (ns, cg[ns], cg[full])
    # no instantiation of the extra inclusions beyond those, and none of their direction kernels
    assert not [n for n in cg if "unused" in n]
    assert sorted(n for n in cg if n.startswith("k_cg_update_ns")) == sorted(t[0] for t in twins)
    # the hot loop's own kernels, pinned where they have been since the 80-SGPR cliff was measured
    assert cg["k_cg_update<0, false, 9, mi::NoFold>"][:2] == (80, 52)
    assert cg["k_cg_pupdate<false, 0, mi::NoFold>"][3] == 0 and cg["k_cg_pupdate<false, 0, mi::NoFold>"][1] <= 64
