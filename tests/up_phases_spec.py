"""f64 specification of the four-phase form of nearest-2x upsampling + 3x3 convolution (fyc_conv_up_phases, include/fyc.h).
A helper, not a test module: tests/test_up_phases.py (CPU) and tests/test_up_phases_gpu.py use it.

The reference reads the SAME packed, storage-rounded phase weights as the kernel (unpack below), so kernel and reference start from the same operand
values and the project's derived bound holds as it stands: |got - ref| <= ulp_T(ref) + (K + 8) 2^-24 S with K = 4 Cin (tests/kernel_compare.py)."""
import torch
import torch.nn.functional as F


def unpack(w_ph: torch.Tensor, slab: int = 64) -> torch.Tensor:
    """packed [4][O][slab][tap = 2 ty + tx][c in slab] -> (4, O, I_pad, 2, 2) f64"""
    P, O, K = w_ph.shape
    Ip = K // 4
    return w_ph.double().reshape(P, O, Ip // slab, 2, 2, slab).permute(0, 1, 2, 5, 3, 4).reshape(P, O, Ip, 2, 2)


def phase_conv(x: torch.Tensor, w4: torch.Tensor, bias=None) -> torch.Tensor:
    """x [frames][Hin][Win][C] f64, w4 (4, O, C, 2, 2) f64 -> [frames][2 Hin][2 Win][O]: output pixel (2 y + py, 2 x + px) is the 2x2 filter of phase
    2 py + px over the input pixels (y - 1 + py + ty, x - 1 + px + tx), zero outside the image"""
    n, H, W, C = x.shape
    O = w4.shape[1]
    xp = F.pad(x.permute(0, 3, 1, 2), (1, 1, 1, 1))
    out = torch.zeros(n, O, 2 * H, 2 * W, dtype=torch.float64)
    for py in range(2):
        for px in range(2):
            full = F.conv2d(xp, w4[2 * py + px])                     # (H + 1) x (W + 1) windows of the padded image
            out[:, :, py::2, px::2] = full[:, :, py:py + H, px:px + W]
    if bias is not None:
        out = out + bias.double().reshape(1, O, 1, 1)
    return out.permute(0, 2, 3, 1).contiguous()


def output_row(m: int, G: int, Hin: int, Win: int) -> int:
    """virtual row m = [group][phase][row in group] -> row of the output tensor, with the kernel's arithmetic: 4 q - 2 x + 2 py Win + px"""
    vs, r = divmod(m, G)
    group, phase = divmod(vs, 4)
    q = group * G + r                       # input pixel, frame-major
    return 4 * q - 2 * (q % Win) + 2 * (phase >> 1) * Win + (phase & 1)


def output_row_by_definition(m: int, G: int, Hin: int, Win: int) -> int:
    vs, r = divmod(m, G)
    group, phase = divmod(vs, 4)
    fr, rem = divmod(group * G + r, Hin * Win)
    y, x = divmod(rem, Win)
    return (fr * 2 * Hin + 2 * y + (phase >> 1)) * 2 * Win + 2 * x + (phase & 1)
