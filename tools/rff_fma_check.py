"""What does torch's CPU matmul compute for RffNet's short contraction (fl32(2 pi) x) b^T?

    python tools/rff_fma_check.py

For dim_in = 1 .. 8 the product is emulated two ways in float64 (a product of two float32 values is exact there) and
rounded to float32 after every step: as a chain of fused multiply-adds in axis order from 0, which is what csrc/rff.hip
computes, and as separately rounded products and sums.  Prints the share of elements each emulation reproduces bit for bit
and the largest distance of each form from the float64 product.  CPU only."""
import numpy as np
import torch


def main():
    torch.manual_seed(0)
    for d in range(1, 9):
        x, b = torch.rand(192, d), torch.randn(128, d) * 10
        v = 2 * np.pi * x
        ref = (v @ b.T).numpy()
        v64, b64, vf, bf = v.double().numpy(), b.double().numpy(), v.numpy(), b.numpy()
        fma, plain = np.zeros((192, 128), np.float32), np.zeros((192, 128), np.float32)
        for k in range(d):
            fma = (v64[:, k:k + 1] * b64[None, :, k] + fma.astype(np.float64)).astype(np.float32)
            plain = plain + (vf[:, k:k + 1] * bf[None, :, k]).astype(np.float32)
        exact = v64 @ b64.T
        print(f"dim_in {d}: FMA chain equals torch on {100 * (fma == ref).mean():.2f} %, separate roundings on "
              f"{100 * (plain == ref).mean():.2f} %; from float64: torch {np.abs(ref - exact).max():.2e}, "
              f"FMA chain {np.abs(fma - exact).max():.2e}, separate {np.abs(plain - exact).max():.2e}")


if __name__ == "__main__":
    main()
