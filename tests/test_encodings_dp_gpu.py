"""Raw ``Image`` payloads cross the data-parallel host ring unconverted: two ranks share the one
card over host-staged gloo (as in tests/test_dp_gpu.py); rank 0 is fed Bayer messages, the ring
step's header says KIND_RAW, rank 1's own live engine converts its shard on the device -- its host
conversion raises if it is used for anything but a calibration sample -- and the gathered
detections are bit-identical to a single-rank run on the same messages."""
import os
import socket

import numpy as np
import pytest
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    os.environ.pop("TCA_DEVICE_ENCODINGS", None)
    import faulthandler
    faulthandler.dump_traceback_later(240, exit=True)  # a hang ends this child, not the session
    try:
        import torch

        from triton_client_amd.inference.engines import LocalDetector2D
        from triton_client_amd.inference.live import LiveCamera
        from triton_client_amd.ops import golden
        from triton_client_amd.parallel.dp import DataParallelDetector2D, init_distributed
        from triton_client_amd.parallel import ring_dp  # noqa: I001  (after dp, which it is imported through)
        from triton_client_amd.ros import msgs
        from triton_client_amd.utils.synthetic import camera_frame

        info = init_distributed("gloo")
        d2 = LocalDetector2D(batch=2, device=info.device)
        dp2 = DataParallelDetector2D(d2, info, max_det=300)
        if info.is_main:
            H, W, enc = 360, 640, "bayer_rggb8"
            step = W + 3
            ims = [msgs.Image(header=msgs.Header(seq=i + 1), height=H, width=W, encoding=enc, step=step,
                              data=golden.rgb8_to_encoding(camera_frame(H, W, 100 + i), enc, step)) for i in range(5)]
            assert dp2._prepare(ims[0])[0] == (ring_dp.KIND_RAW, H, W, golden.IMAGE_ENCODINGS[enc], step, 0)
            got = dp2.process(ims, draw=False)
            dp2.close()
            want = d2.live().process(ims, draw=False)  # the single-rank run
            assert all(len(d) > 0 for _, d in want)
            for (_, g), (_, w) in zip(got, want):
                np.testing.assert_array_equal(g, w)
            # and those are the detections of the specification's pixels
            ref = d2.detect([golden.image_to_rgb8(m.data, H, W, step, enc) for m in ims])
            for (_, g), r in zip(got, ref):
                np.testing.assert_array_equal(g, r)
            q.put((0, "ok"))
        else:
            def no_host(*a, **k):
                raise AssertionError("worker rank used the host detect() path")
            d2.detect = no_host
            host_rgb = LiveCamera.host_rgb

            def guarded(m, hw=None):
                if d2.calibrate_target is None:  # not a calibration sample
                    raise AssertionError("worker rank converted an Image on the host")
                return host_rgb(m, hw)
            LiveCamera.host_rgb = staticmethod(guarded)
            kinds, serve_step = [], dp2._serve_step

            def recorded(hdr, items, view):
                kinds.append(int(hdr[ring_dp.H_KIND]))
                return serve_step(hdr, items, view)
            dp2._serve_step = recorded
            n = dp2.serve()
            raw = [e.kind for e in d2.live().engines.values()]
            q.put((rank, f"served {n} kinds {kinds} engines {raw}"))
        torch.cuda.synchronize()
        q.close()
        q.join_thread()
        os._exit(0)
    except Exception:  # pragma: no cover
        import traceback
        q.put((rank, traceback.format_exc()))
        q.close()
        q.join_thread()
        os._exit(1)


def test_raw_images_cross_the_ring_unconverted(cuda):
    from triton_client_amd.parallel import dp  # noqa: F401  (ring_dp is imported through it)
    from triton_client_amd.parallel.ring_dp import KIND_RAW

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=300) for _ in range(2))
    for p in procs:
        p.join(timeout=60)
        if p.is_alive():
            p.kill()
    assert res == {0: "ok", 1: f"served 1 kinds [{KIND_RAW}] engines ['raw']"}, res
