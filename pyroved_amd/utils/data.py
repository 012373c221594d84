"""DataLoader helpers with the call signatures of pyroved/utils/data.py:6-52.

Behaviour contract kept from the reference (it defines the data order parity depends on):
`TensorDataset(*tensors)`, batch_size 100 unless given, `shuffle=True` unless a `RandomSampler` is asked for,
a `torch.Generator(device)` handed to the loader only when `device=` is passed.  SVItrainer recognises loaders
built here (plain TensorDataset + standard samplers) and feeds them from device memory (trainers/svi.py).
"""
import math
from typing import Iterator, Tuple

import torch
from torch.utils.data import DataLoader, RandomSampler, TensorDataset


def init_dataloader(*args: torch.Tensor, random_sampler: bool = False, shuffle: bool = True,
                    **kwargs: int) -> DataLoader:
    """DataLoader over the given tensors.  kwargs: batch_size (100), device (generator device)."""
    dev = kwargs.get("device")
    opts = dict(batch_size=kwargs.get("batch_size", 100),
                generator=torch.Generator(dev) if dev else None)
    ds = TensorDataset(*args)
    if random_sampler:
        opts["sampler"] = RandomSampler(ds)
    else:
        opts["shuffle"] = shuffle
    return DataLoader(ds, **opts)


def weights_from_nan(x, fill: float = 0.0) -> Tuple[torch.Tensor, torch.Tensor]:
    """Missing values marked by NaN -> (x_filled, w): x with every NaN replaced by `fill`, and w of x's shape and (floating)
    dtype with 0 where x was NaN and 1 elsewhere.  The front door of SVItrainer(model, image_weights=True) for NaN-marked data:
    the encoder sees x as given, so x itself must be finite everywhere — `fill` is what the encoder sees at the missing
    positions; the likelihood ignores them (weight 0).  x: a tensor or an ndarray; neither is modified.

        x, w = weights_from_nan(scan)                      # scan: (n, *data_dim) with NaN where nothing was measured
        loader = init_dataloader(x, w, batch_size=64)      # the weights travel as the batches' last tensor
        trainer = SVItrainer(model, image_weights=True)"""
    t = torch.as_tensor(x)
    if not t.is_floating_point():
        t = t.to(torch.float32)
    if not math.isfinite(float(fill)):
        raise ValueError("fill must be finite (got %r): the encoder reads the filled values" % (fill,))
    missing = torch.isnan(t)
    w = (~missing).to(t.dtype)
    return torch.where(missing, torch.full_like(t, float(fill)), t), w


def onehot_channels(labels, num_classes: int) -> torch.Tensor:
    """Integer label images (n, *dims) -> channel-last float32 one-hot (n, *dims, num_classes): the data of
    iVAE(data_dim, ..., channels=num_classes, sampler_d="categorical", sigmoid_d=False).  labels: a tensor or an ndarray of an
    integer dtype with every entry in 0 .. num_classes - 1 (ValueError otherwise); it is not modified."""
    t = torch.as_tensor(labels)
    if t.is_floating_point() or t.is_complex() or t.dtype == torch.bool:
        raise ValueError("labels must have an integer dtype (got %s)" % t.dtype)
    if isinstance(num_classes, bool) or int(num_classes) != num_classes or num_classes < 1:
        raise ValueError("num_classes must be a positive int (got %r)" % (num_classes,))
    t = t.to(torch.int64)
    if t.numel() and (int(t.min()) < 0 or int(t.max()) >= num_classes):
        raise ValueError("labels must lie in 0 .. %d (got %d .. %d)" % (num_classes - 1, int(t.min()), int(t.max())))
    out = torch.zeros(*t.shape, int(num_classes), dtype=torch.float32)
    return out.scatter_(-1, t.unsqueeze(-1), 1.0)


def iter_batches(*args: torch.Tensor, batch_size: int = 100) -> Iterator[Tuple[torch.Tensor, ...]]:
    """The batches `init_dataloader(*args, shuffle=False, batch_size=...)` yields — same boundaries, same order, the last
    one partial — as views of the callers' tensors.  The inference loops (encode / decode / predict / classifier) walk
    their input in order, where a DataLoader over a TensorDataset indexes and collates SAMPLE BY SAMPLE on the host
    (0.3-1.5 s per 65 536 images of 28x28, ~50x the kernels' time)."""
    n = args[0].shape[0]
    if any(a.shape[0] != n for a in args):
        raise ValueError("Size mismatch between tensors")          # (TensorDataset's assertion)
    # iter(DataLoader) draws its base seed from the global CPU generator even when nothing is shuffled; an encode /
    # classifier call between two epochs therefore moves the stream the NEXT epoch's permutation and noise come from
    # (the reference trainers' recorded histories include that draw): consume exactly the same value here
    torch.empty((), dtype=torch.int64).random_()
    for lo in range(0, n, batch_size):
        yield tuple(a[lo:lo + batch_size] for a in args)


def init_ssvae_dataloaders(data_unsup: torch.Tensor, data_sup: Tuple[torch.Tensor], data_val: Tuple[torch.Tensor],
                           **kwargs: int) -> Tuple[DataLoader, DataLoader, DataLoader]:
    """(unlabeled, labeled, validation) loaders for the semi-supervised trainers (pyroved/utils/data.py:41-52).
    The reference passes `sampler=True` for the labeled set, a keyword its init_dataloader swallows in **kwargs —
    i.e. all three are plain shuffling loaders; kept so."""
    return (init_dataloader(data_unsup, **kwargs),
            init_dataloader(*data_sup, **kwargs),
            init_dataloader(*data_val, **kwargs))
