"""The arithmetic kernel W's table trips rest on (fm_search.hip), on the CPU oracle alone: every row of an SA
interval carries one BWT symbol A/C/G/T except the primary row, so

    width(parent) = sum of the widths of its four children + [primary row inside the parent's interval],

and exactly one key of every level -- the indexed text's own prefix -- holds the primary row."""
import numpy as np
import pytest

import nabwa_testlib as T
import width_cases as W

DEPTH = 6


@pytest.fixture(scope="module")
def olib():
    return T.load_oracle()


@pytest.fixture(scope="module")
def oix(olib):
    return T.OracleIndex(olib)


@pytest.mark.parametrize("which", [0, 1])
def test_parent_width_is_the_sum_of_its_children_plus_the_primary_row(olib, oix, which):
    primary, _, seq_len = W.bwt_header(oix.bwt(which))
    lv = W.oracle_levels(olib, oix.bwt(which), DEPTH + 1)
    assert lv[0][0, 1] - lv[0][0, 0] + 1 == seq_len + 1
    for t in range(1, DEPTH + 1):
        par, kids = lv[t], lv[t + 1]
        assert len(par) == 4 ** t and len(kids) == 4 ** (t + 1)
        holds = (par[:, 0] <= par[:, 1]) & (par[:, 0] <= primary) & (primary <= par[:, 1])
        assert int(holds.sum()) == 1, "level %d: %d keys hold the primary row" % (t, int(holds.sum()))
        child_sum = W.widths(kids).reshape(-1, 4).sum(axis=1)
        assert np.array_equal(W.widths(par), child_sum + holds), "level %d" % t
        # what the kernel hands on for a summed level: {1, sum} is empty exactly where the entry is
        assert np.array_equal(child_sum + holds == 0, par[:, 0] > par[:, 1])


@pytest.mark.parametrize("which", [0, 1])
def test_the_primary_key_is_the_text_prefix_in_consumption_order(olib, oix, which):
    """the key that holds the primary row at level t spells the first t bases of the indexed text, the LAST of them consumed
    first: bwt[0] indexes the genome, bwt[1] the genome reversed"""
    primary, _, _ = W.bwt_header(oix.bwt(which))
    text = "".join(W.toy_contigs())
    if which:
        text = text[::-1]
    lv = W.oracle_levels(olib, oix.bwt(which), DEPTH)
    for t in range(1, DEPTH + 1):
        key = 0
        for ch in text[:t][::-1]:
            key = 4 * key + "ACGT".index(ch)
        k, l = lv[t][key]
        assert k <= primary <= l, (t, key)
