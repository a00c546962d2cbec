"""What the per-frame GPU tests (LPC, statistics, pitch, test_gpu_frame_src.py)
share: the frame gather they compare the fused entry points with, and their
signals and window.  numpy only at import; torch is imported where it is used.
"""
import ctypes as C

import numpy as np

_vp, _sz = C.c_void_p, C.c_size_t
OK = 0


def fetch_frames(vdev, ch, frame, hop, center, window, frames=None):
    """vv_dsp_fetch_frames_device of one contiguous channel -> (frames, frame);
    frames: how many, from frame 0 (None: num_frames of the channel)"""
    import torch
    L = vdev.lib()
    L.vv_dsp_fetch_frames_device.argtypes = [_vp, _sz, _vp, _sz, _sz, _sz, _sz, C.c_int, _vp, _vp]
    fr = vdev.num_frames(ch.numel(), frame, hop, center) if frames is None else frames
    out = torch.empty((fr, frame), dtype=torch.float32, device=ch.device)
    st = L.vv_dsp_fetch_frames_device(ch.data_ptr(), ch.numel(), out.data_ptr(), frame, hop, 0, fr, int(center),
                                      None if window is None else window.data_ptr(),
                                      torch.cuda.current_stream().cuda_stream)
    assert st == OK
    return out


def three_channels(white, resonant):
    """(3, 16000) view of a (3, 16004) buffer: ch_stride 16004"""
    import torch
    buf = torch.zeros((3, 16004), dtype=torch.float32, device="cuda")
    for i, s in enumerate((white, resonant, white[::-1].copy())):
        buf[i, :16000] = torch.from_numpy(s).cuda()
    return buf[:, :16000]


def hamming(n):
    """0.54 - 0.46 cos(2 pi i / (n - 1)) rounded to float32; ones for n = 1"""
    if n == 1:
        return np.ones(1, np.float32)
    return (0.54 - 0.46 * np.cos(2.0 * np.pi * np.arange(n) / (n - 1))).astype(np.float32)
