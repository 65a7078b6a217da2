"""HGTLayer's train-mode dropout mask (models/HGT.py): counter-based under an active dropout seed base - the draw a captured step can replay -
and torch's generator draw otherwise."""
import torch


def _layer(p=0.2):
    from wsi_hgnn_amd.models.HGT import HGTLayer
    layer = HGTLayer(8, 8, {"0": 0}, {("0", "e", "0"): 0}, 2, dropout=p)
    return layer.train()


def test_mask_under_a_seed_base_is_the_counter_based_draw(monkeypatch):
    """What the layer asks ``ops.dropout_apply`` for is a table of ones under ``CounterDropout(p, next host seed, the active base)``: the mask
    is ``ops.dropout_keep_mask`` of that (p, seed, base), scaled by 1 / (1 - p).  (The kernel itself is held against ``dropout_keep_mask`` on the
    GPU.)"""
    from wsi_hgnn_amd import ops
    base = torch.tensor([-123456789], dtype=torch.int32)
    seen = []

    def apply(x, drop, row0=0):
        seen.append((x.clone(), drop))
        return x * ops.dropout_keep_mask(drop, x.shape[0], x.shape[1], x.device, row0).to(x.dtype) * torch.tensor(drop.scale, dtype=x.dtype)

    monkeypatch.setattr(ops, "current_dropout_seed_base", lambda device: base)
    monkeypatch.setattr(ops, "next_dropout_seed", lambda: 777)
    monkeypatch.setattr(ops, "dropout_apply", apply)
    layer = _layer(0.2)
    h = torch.randn(37, 8)
    before = torch.get_rng_state()
    mask = layer._dropout_mask(h)
    assert torch.equal(torch.get_rng_state(), before)                 # torch's generator is not touched
    (x, drop), = seen
    assert x.shape == h.shape and bool((x == 1).all())
    assert (drop.p, drop.seed, drop.seed_base) == (0.2, 777, base) and drop.seed_base is base
    want = ops.dropout_keep_mask(ops.CounterDropout(0.2, 777, base), 37, 8).to(torch.float32) * torch.tensor(1.0 / (1.0 - 0.2), dtype=torch.float32)
    assert torch.equal(mask, want)
    assert set(mask.unique().tolist()) == {0.0, 1.25} and 0.05 < float((mask == 0).float().mean()) < 0.4
    # another value of the device word: another mask from the same host seed
    base.add_(ops.SEED_STRIDE)
    assert not torch.equal(layer._dropout_mask(h), mask)


def test_mask_without_a_seed_base_is_the_generator_draw(monkeypatch):
    from wsi_hgnn_amd import ops
    monkeypatch.setattr(ops, "dropout_apply", lambda *a, **k: (_ for _ in ()).throw(AssertionError("counter-based draw without a seed base")))
    layer = _layer(0.2)
    h = torch.randn(23, 8)
    assert ops.current_dropout_seed_base(h.device) is None
    torch.manual_seed(5)
    mask = layer._dropout_mask(h)
    torch.manual_seed(5)
    want = torch.empty_like(h).bernoulli_(0.8).mul_(1.0 / 0.8)
    assert torch.equal(mask, want)
    assert bool((_layer(1.0)._dropout_mask(h) == 0).all())
