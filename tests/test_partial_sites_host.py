"""``engine.PartialSites`` without a GPU: the registry of the launch sites that leave partial rows in buffers of their own.  The order
of its job list is part of deterministic mode's contract (the order of the totals inside an ordered-reduce chain), so it is pinned
here on CPU tensors."""

from __future__ import annotations

import pytest
import torch

from maestro_amd import hip
from maestro_amd.engine import PartialSites


def _site(rows: int, dst: torch.Tensor, calls: list | None = None):
    def make():
        if calls is not None:
            calls.append(rows)
        buf = torch.zeros(rows, 4)
        return buf, [(buf.view(-1), dst, rows, 4, 4)]
    return make


def _sources(jobs) -> list:
    return [j[0].data_ptr() for j in jobs]


def test_jobs_come_back_in_first_launch_order_and_keys_select_without_reordering():
    sites, dst = PartialSites(capturing=lambda: False), torch.zeros(4)
    order = [("ln_enc", "z"), ("embed", "a"), ("ln_dec", "m"), ("tok", "b")]         # neither sorted nor reverse sorted
    bufs = {key: sites.get("bwd", key, _site(i + 1, dst)) for i, key in enumerate(order)}
    other = sites.get("fwd", ("loss", "a"), _site(9, dst))
    assert [k for k, _ in sites.items("bwd")] == order and sites.items("fwd") == [(("loss", "a"), other)]
    assert _sources(sites.jobs("bwd")) == [bufs[k].data_ptr() for k in order]
    assert [j[2] for j in sites.jobs("bwd")] == [1, 2, 3, 4] and [j[2] for j in sites.jobs("fwd")] == [9]
    picked = sites.jobs("bwd", keys=[("tok", "b"), ("ln_enc", "z")])                  # named in the opposite order
    assert _sources(picked) == [bufs[("ln_enc", "z")].data_ptr(), bufs[("tok", "b")].data_ptr()]
    assert sites.jobs("bwd", keys=[("ln_joint", "z")]) == [] and sites.jobs("none") == []
    assert sorted(t.data_ptr() for t in sites.buffers()) == sorted([other.data_ptr()] + [b.data_ptr() for b in bufs.values()])


def test_a_changed_variant_replaces_the_site_in_place_and_an_unchanged_one_is_kept():
    sites, dst, calls = PartialSites(capturing=lambda: False), torch.zeros(4), []
    first = sites.get("bwd", ("rec", "a"), _site(1, dst, calls))
    old = sites.get("bwd", ("tok", "a"), _site(2, dst, calls), variant=False)
    last = sites.get("bwd", ("embed", "a"), _site(3, dst, calls))
    sites.tables["bwd"], sites.tables["fwd"] = "reducer of the backward", "reducer of the forward"
    assert sites.get("bwd", ("tok", "a"), _site(7, dst, calls), variant=False) is old and calls == [1, 2, 3]
    assert sites.tables["bwd"] == "reducer of the backward"
    new = sites.get("bwd", ("tok", "a"), _site(5, dst, calls), variant=True)
    assert calls == [1, 2, 3, 5] and new is not old and new.shape[0] == 5
    assert [k for k, _ in sites.items("bwd")] == [("rec", "a"), ("tok", "a"), ("embed", "a")]
    assert _sources(sites.jobs("bwd")) == [first.data_ptr(), new.data_ptr(), last.data_ptr()]
    assert old.data_ptr() not in _sources(sites.jobs("bwd")) and old.data_ptr() not in [t.data_ptr() for t in sites.buffers()]
    assert "bwd" not in sites.tables and sites.tables["fwd"] == "reducer of the forward"
    assert sites.get("bwd", ("tok", "a"), _site(8, dst, calls), variant=True) is new and calls == [1, 2, 3, 5]


def test_a_site_is_not_built_inside_a_capture_and_dict_buffers_are_listed():
    capturing = [True]
    sites, dst = PartialSites(capturing=lambda: capturing[0]), torch.zeros(4)
    with pytest.raises(hip.HipExtensionError, match="capture"):
        sites.get("bwd", ("rec", "a"), _site(1, dst))
    assert sites.jobs("bwd") == []
    capturing[0] = False
    slabs, cs = torch.zeros(2, 4), torch.zeros(1, 4)
    w = sites.get("bwd", ("rec", "a"), lambda: (dict(slabs=slabs, cs=cs), [(slabs.view(-1), dst, 2, 4, 4), (cs.view(-1), dst, 1, 4, 4)]))
    capturing[0] = True                 # a replayed or captured launch of a known site only looks it up
    assert sites.get("bwd", ("rec", "a"), _site(1, dst)) is w
    assert [t.data_ptr() for t in sites.buffers()] == [slabs.data_ptr(), cs.data_ptr()] and len(sites.jobs("bwd")) == 2
