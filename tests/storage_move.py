"""Shared by the GPU tests of the graphed runners: parameter storage that moves WITHOUT GraphedStep (whose set-up repoints the
pack cache itself), with new values, so that a capture which re-packs from the old addresses gives old numbers."""
import torch


def move_two_weights(m, seed=9):
    """`p.data = old + delta` for two weights the pack cache reads through different pointer tables: the first convolution's
    (3 input channels: the generic table) and a 3x3 one whose channel counts are both multiples of 32 (the tiled table,
    PackCache._table3).  The model must have run once, so that both tables exist.  Returns the old tensors: while the caller
    holds them, the old addresses stay valid memory holding the old values, whatever the allocator does."""
    convs = [p for p in m.parameters() if p.dim() == 4 and tuple(p.shape[2:]) == (3, 3)]
    first, tiled = convs[0], next(p for p in convs if p.shape[0] % 32 == 0 and p.shape[1] % 32 == 0)
    assert first.shape[1] == 3 and first is not tiled
    assert m._pack_cache._table is not None and m._pack_cache._n3 > 0
    g, kept = torch.Generator().manual_seed(seed), []
    for p in (first, tiled):
        old = p.data
        kept.append(old)
        p.data = old + 0.05 * torch.randn(p.shape, generator=g).to(old.device)
        assert p.data_ptr() != old.data_ptr()
    return kept


def twin_of(m, make):
    """a second model holding m's values on storage and a pack cache of its own: the moved model's own eager forward reads
    its weights through the pack cache under test, so the expectation comes from here"""
    twin = make()
    twin.load_state_dict(m.state_dict())
    return twin
