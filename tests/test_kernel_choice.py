"""Every plan step's kernel and every conv's fragment-weight bytes, pinned (tests/golden/kernel_choice.json, written by
tools/make_kernel_choice.py): kernel selection is decided once per plan, at creation, from the plan's options; a change to
what any step of the matrix runs shows up here, on a machine without a GPU."""
import json

import pytest
import torch

import kernel_choice_util as kc


@pytest.mark.skipif(torch.cuda.is_available(), reason="fake device addresses must never reach a library that can launch")
def test_kernel_choice_pinned():
    with open(kc.FIXTURE) as fh:
        want = json.load(fh)
    got = kc.all_choices()
    assert sorted(got["configs"]) == sorted(want["configs"])
    bad = []
    for key in want["configs"]:
        w, g = kc.config_rows(want, key), kc.config_rows(got, key)
        if g != w:
            bad.append((key, [(n, a, b) for n, (a, b) in enumerate(zip(w, g)) if a != b][:4]))
    assert not bad, "%d of %d configurations changed, e.g. %s" % (len(bad), len(want["configs"]), bad[:5])
