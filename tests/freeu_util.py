"""Shared pieces of the FreeU tests: diffusers 0.24's `fourier_filter` / `apply_freeu` restated with torch.fft (the reference form),
the FFT-free seven-basis form the kernel evaluates (float64), and forward-pre-hooks that put FreeU into the oracle UNet."""
import math

import torch

FREEU = dict(s1=0.9, s2=0.2, b1=1.2, b2=1.4)
PLANES = [(1, 1), (1, 2), (2, 1), (1, 5), (4, 1), (2, 2), (3, 3), (7, 10), (16, 16), (64, 64)]


def fourier_filter_fft(x, threshold, scale):
    """diffusers 0.24 `fourier_filter` on [..., h, w]: fftn over (h, w), fftshift, the centre box times `scale`, back, real part."""
    h, w = x.shape[-2:]
    f = torch.fft.fftshift(torch.fft.fftn(x.to(torch.complex128 if x.dtype == torch.float64 else torch.complex64), dim=(-2, -1)), dim=(-2, -1))
    mask = torch.ones(x.shape[-2:], dtype=f.real.dtype)
    crow, ccol = h // 2, w // 2
    mask[crow - threshold:crow + threshold, ccol - threshold:ccol + threshold] = scale      # (Python slices: -1:1 on a 1-pixel axis is its only row)
    f = f * mask
    return torch.fft.ifftn(torch.fft.ifftshift(f, dim=(-2, -1)), dim=(-2, -1)).real.to(x.dtype)


def trig_basis(h, w, dtype=torch.float64):
    """[7, h, w]: 1, cos ty, sin ty, cos tx, sin tx, cos(ty + tx), sin(ty + tx); the cos / sin of a 1-pixel axis are zero."""
    ty = (2.0 * math.pi * torch.arange(h, dtype=torch.float64) / h)[:, None].expand(h, w)
    tx = (2.0 * math.pi * torch.arange(w, dtype=torch.float64) / w)[None, :].expand(h, w)
    zero = torch.zeros(h, w, dtype=torch.float64)
    cy, sy = (torch.cos(ty), torch.sin(ty)) if h > 1 else (zero, zero)
    cx, sx = (torch.cos(tx), torch.sin(tx)) if w > 1 else (zero, zero)
    return torch.stack([torch.ones(h, w, dtype=torch.float64), cy, sy, cx, sx, cy * cx - sy * sx, sy * cx + cy * sx]).to(dtype)


def fourier_filter_basis(x, scale):
    """y = x + (scale - 1) / hw * sum_k (sum_pixels x phi_k) phi_k on [..., h, w], float64."""
    h, w = x.shape[-2:]
    phi = trig_basis(h, w)
    x = x.double()
    sums = torch.einsum("...hw,khw->...k", x, phi)
    return x + (scale - 1.0) / (h * w) * torch.einsum("...k,khw->...hw", sums, phi)


def apply_freeu_torch(hidden, skip, b, s):
    """diffusers 0.24 `apply_freeu` for one resolution index on NCHW tensors."""
    hidden = hidden.clone()
    hidden[:, :hidden.shape[1] // 2] = hidden[:, :hidden.shape[1] // 2] * b
    return hidden, fourier_filter_fft(skip, 1, s)


def hook_oracle(ref, s1, s2, b1, b2):
    """Forward-pre-hooks on up_blocks[0..1].resnets[j] of the oracle UNet: split the concatenated input at the hidden width (the
    previous stage's output width for j = 0, the block's own otherwise) and apply the torch restatement.  Returns the handles."""
    handles = []
    prev = ref.mid_block.resnets[-1].conv1.out_channels
    for i, blk in enumerate(ref.up_blocks):
        own = blk.resnets[0].conv1.out_channels
        if i < 2:
            b, s = (b1, s1) if i == 0 else (b2, s2)
            for j, res in enumerate(blk.resnets):
                width = prev if j == 0 else own

                def pre(_mod, args, width=width, b=b, s=s):
                    x = args[0]
                    hidden, skip = apply_freeu_torch(x[:, :width], x[:, width:], b, s)
                    return (torch.cat([hidden, skip], dim=1),) + tuple(args[1:])

                handles.append(res.register_forward_pre_hook(pre))
        prev = own
    return handles
