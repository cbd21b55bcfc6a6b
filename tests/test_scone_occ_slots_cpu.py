"""SconeOcc._grad_slots(): where each of the 172 parameters lies in the 140-entry weight table, and the backward-mode switch (no GPU)."""
import pytest
import torch


@pytest.fixture(scope="module")
def occ():
    from macarons_amd.networks import SconeOcc
    return SconeOcc()


def _shapes(occ):
    """the table's shapes, from the parameters alone: every entry is a parameter or the w_q | w_k | w_v rows stacked"""
    return [tuple(t.shape) for t in occ.weight_table()]


def test_slots_cover_every_parameter_with_its_shape(occ):
    params, slots = occ._grad_slots()
    assert len(params) == len(slots) == 172 == len(list(occ.parameters()))
    table = [torch.zeros(s) for s in _shapes(occ)]
    assert len(table) == 140
    for p, (k, rows) in zip(params, slots):
        assert 0 <= k < 140
        piece = table[k] if rows is None else table[k][rows[0]:rows[1]]
        assert tuple(piece.shape) == tuple(p.shape), (k, rows, tuple(p.shape))


def test_slots_tile_every_table_entry(occ):
    params, slots = occ._grad_slots()
    shapes = _shapes(occ)
    cover = [torch.zeros(s[0], dtype=torch.int32) for s in shapes]
    for k, rows in slots:
        if rows is None:
            cover[k] += 1
        else:
            cover[k][rows[0]:rows[1]] += 1
    for k, c in enumerate(cover):
        assert bool((c == 1).all()), f"table entry {k}: rows covered {sorted(set(c.tolist()))} times"
    # the packed entries are cut at 32 | 64 | 192
    packed = sorted({(k, rows) for k, rows in slots if rows is not None})
    assert len(packed) == 4 * 2 * 2 * 3 and {rows for _, rows in packed} == {(0, 32), (32, 64), (64, 192)}


def test_slot_order_is_the_weight_tables(occ):
    params, slots = occ._grad_slots()
    with torch.no_grad():
        saved = [p.clone() for p in params]
        try:
            for j, p in enumerate(params):
                p.fill_(float(j + 1))
            table = occ.weight_table()
            for j, (p, (k, rows)) in enumerate(zip(params, slots)):
                piece = table[k] if rows is None else table[k][rows[0]:rows[1]]
                assert bool((piece == float(j + 1)).all()), (j, k, rows)
        finally:
            for p, s in zip(params, saved):
                p.copy_(s)


def test_a_parameter_outside_the_table_is_refused():
    from macarons_amd.networks import SconeOcc
    m = SconeOcc()
    m.extra = torch.nn.Parameter(torch.zeros(3))
    with pytest.raises(NotImplementedError, match="extra"):
        m._grad_slots()


@pytest.mark.parametrize("value,mode", [(None, "composite"), ("composite", "composite"), ("pct", "pct"), ("hip", "hip"), ("xyz", "composite")])
def test_backward_mode(monkeypatch, value, mode):
    from macarons_amd import autograd as A
    if value is None:
        monkeypatch.delenv("MCR_SCONE_OCC_BWD", raising=False)
    else:
        monkeypatch.setenv("MCR_SCONE_OCC_BWD", value)
    assert A.scone_occ_backward_mode() == mode
