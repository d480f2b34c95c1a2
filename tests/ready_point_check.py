"""The ready-point check of the trainers' flat gradient buffer, shared by the GPU tests.

``CprTrainer`` lays the gradients out in the order the backward pass completes them, and every backward rule calls ``_done(p)`` to say that
the prefix up to ``p`` has been enqueued; the bucketed reducer launches its collective on that word alone.  ``checked(trainer_cls)`` returns a
subclass whose ``_done`` looks at the buffer at that moment: with the buffer filled with NaN before the step, a ready point that fires before
its gradients are written finds a NaN in the prefix it declares.  A drift of this kind is silent on one GPU otherwise."""
import torch


def checked(trainer_cls):
    """-> (the checked subclass of ``trainer_cls``, ``seen``: the prefix ends its ``_done`` has verified, in call order).  The class
    attribute ``check`` (True) switches the check off for later steps of the same trainer."""
    seen = []

    class Checked(trainer_cls):
        check = True

        def _done(self, p):
            if self.check and p.requires_grad:
                end = self.offset[id(p)][1]
                torch.cuda.synchronize()          # what wait_stream(side) + stream order give the collective
                bad = torch.isnan(self.flat_g[:end])
                assert not bool(bad.any()), 'gradient prefix [0, %d) declared final with %d unwritten entries (first at %d)' % (
                    end, int(bad.sum()), int(bad.nonzero()[0]))
                seen.append(end)
            super()._done(p)
    return Checked, seen


def run_checked_backward(trainer_cls, model, data, **trainer_kw):
    """One forward_backward of the checked trainer on a NaN-filled buffer, with the assertions every ready-point test makes: no NaN in a
    declared prefix (inside ``_done``), the whole buffer written at the end, the ready points sweep the buffer front to back and reach its
    end.  -> (the trainer, seen)."""
    cls, seen = checked(trainer_cls)
    tr = cls(model, **trainer_kw)
    tr.flat_g.fill_(float('nan'))
    tr.forward_backward(**data)
    torch.cuda.synchronize()
    assert not bool(torch.isnan(tr.flat_g).any()), 'some trainable parameter never received a gradient'
    assert bool(torch.isfinite(tr.flat_g).all())
    assert seen and max(seen) == tr.flat_g.numel() and seen == sorted(seen), 'ready points must sweep the buffer front to back'
    return tr, seen
