"""References of a 2-D Fourier transform and of the reference's log-magnitude spectrum that run anywhere numpy does:

  get_fft           the numpy restatement of the reference's im_helpers.get_fft, the same calls in the same order.  numpy transforms a
                    float32 image in SINGLE precision (np.fft.fft2 of float32 is complex64 since numpy 2.0), so the reference's float32
                    output is its own complex64 arithmetic rounded, several float32 ulp from the exact spectrum; the golden file
                    stores how far (ref_ulps): a device form computing in float64 is to be held to one ulp of the truth and to that distance plus one of the reference.
  dft2_longdouble   an independent O(n^2) DFT-matrix transform in longdouble: no factorisation, no butterflies, no library.
  spectrum, shift, to_uint8, bounds   the definitions the tests share."""
import numpy as np


def get_fft(frame: np.ndarray) -> np.ndarray:
    fft = np.fft.fft2(frame[..., 0])
    fshift = np.fft.fftshift(fft)
    with np.errstate(divide="ignore", invalid="ignore"):
        magnitude_spectrum = 20 * np.log(np.abs(fshift))
        magnitude_rgb = np.zeros_like(frame)
        magnitude_rgb[..., 0] = magnitude_spectrum
    return magnitude_rgb


def dft_matrix(n: int) -> np.ndarray:
    """exp(-2 pi i j k / n) in longdouble, the exponent reduced modulo n in integers"""
    pi = 4 * np.arctan(np.longdouble(1))
    jk = (np.arange(n)[:, None] * np.arange(n)[None, :]) % n
    ang = 2 * pi * jk.astype(np.longdouble) / np.longdouble(n)
    return np.cos(ang) - 1j * np.sin(ang)


def dft2_longdouble(plane: np.ndarray) -> np.ndarray:
    """(H, W) real -> (H, W) complex longdouble"""
    H, W = plane.shape
    x = plane.astype(np.longdouble).astype(np.clongdouble)
    return dft_matrix(H) @ x @ dft_matrix(W)


def full_from_half(half: np.ndarray, W: int) -> np.ndarray:
    """the full (H, W) spectrum of a real image from its columns 0 .. W // 2: F[(H - y) % H][(W - x) % W] = conj(F[y][x])"""
    H = half.shape[0]
    full = np.empty((H, W), half.dtype)
    full[:, :W // 2 + 1] = half
    ys = (H - np.arange(H)) % H
    for x in range(W // 2 + 1, W):
        full[:, x] = np.conj(half[ys, W - x])
    return full


def shift(a: np.ndarray) -> np.ndarray:
    """index k goes to (k + n // 2) % n on the last two axes (np.fft.fftshift)"""
    H, W = a.shape[-2:]
    out = np.empty_like(a)
    out[..., (np.arange(H)[:, None] + H // 2) % H, (np.arange(W)[None, :] + W // 2) % W] = a
    return out


def spectrum(F: np.ndarray) -> np.ndarray:
    """20 ln|F|, shifted, float64"""
    with np.errstate(divide="ignore"):
        return shift(20 * np.log(np.abs(F)))


def to_uint8(s: np.ndarray) -> np.ndarray:
    """truncate toward zero, then modulo 256 (finite values only: no fixture holds another)"""
    assert np.isfinite(s).all()
    return (np.trunc(s).astype(np.int64) & 255).astype(np.uint8)


def rms(F: np.ndarray) -> float:
    return float(np.sqrt(np.mean(np.abs(F) ** 2)))


def complex_bound(numpy_err: float) -> float:
    """g of a case: 4 x numpy's own stored error, and not below 4 x 2^-52"""
    return 4.0 * max(float(numpy_err), 2.0 ** -52)


def spectrum_bound(F_true: np.ndarray, g: float) -> np.ndarray:
    """per bin (shifted): 20 g rms|F| / |F[bin]| plus 64 ulp of s"""
    s = spectrum(F_true)
    return shift(20.0 * g * rms(F_true) / np.abs(F_true)) + 64 * np.spacing(np.abs(s))


def ulps_f32(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """distance in float32 ulp between two finite float32 arrays"""
    def key(x):
        i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))
