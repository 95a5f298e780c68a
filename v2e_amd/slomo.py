"""Drop-in `SuperSloMo` running the interpolation network on MI355X HIP kernels.

Mirrors v2ecore/slomo.py: constructor signature (:44-54), `interpolate(source_frame_path,
output_folder, frame_size) -> (interpTimes, avgUpsampling)` writing `<idx>.png` (:231-495),
`get_interpolated_timestamps` (:540-564), `cleanup`.  The two UNets, the backWarp
grid-sample, the flow blends and the fusion (slomo.py:338-345, 404-433; model.py:10-300) run
in libv2e_amd.so (f32 MFMA implicit-GEMM convolutions); PyTorch only owns the buffers.

Differences from the reference, all at the edges of the hot path:
  * all `upsampling_factor` time points of a batch go through the interpolation UNet as one
    batch (n_t * B samples) instead of a Python loop -- same arithmetic per sample;
  * the AVI / preview writers (slomo.py:288-303, 447-490) are host work outside the hot path: `video_path`, `vid_orig`,
    `vid_slomo` and `preview` are accepted as the reference's CLI passes them (v2e.py:471-478); the two AVIs are written on the
    host through cv2 when cv2 is importable and skipped with ONE warning when it is not -- the constructor never raises for
    them, and the interpolation itself is unaffected;
  * host-side pre/post-processing (PIL LANCZOS / BILINEAR resize, PNG files) is kept as is.

Here: the file-based class with its writers, preview, checkpoint loading and first-batch self-check.  The device side is
`slomo_engine.SloMoEngine` on two `unet.HipUNet`s, the batch arithmetic `planning`'s; their names are re-exported here.
"""
import atexit
import weakref
import glob
import logging
import os

import numpy as np
import torch

from . import _capi
from ._capi import check, ptr, stream_ptr
from .planning import _batch_interp_times, factor_from_speed, speed_from_bits, time_coefficients, time_points  # noqa: F401  (re-exported)
from .slomo_engine import SloMoEngine
from .unet import UNET_LAYERS, HipUNet, weight_scale_log2  # noqa: F401  (re-exported)

logger = logging.getLogger(__name__)

OUTPUT_VIDEO_CODEC_FOURCC = 'XVID'  # v2ecore/v2e_utils.py:22, the codec of video_writer


def _all_images(data_path):
    """slomo.py:500-521: the PNGs of a folder in numerical order."""
    images = glob.glob(os.path.join(data_path, '*.png'))
    if len(images) == 0:
        raise ValueError("Input folder is empty or images are not in 'png' format.")
    return sorted(images, key=lambda line: int(line.split(os.sep)[-1].split('.')[0]))


def _cleanup_at_exit(ref):
    obj = ref()
    if obj is not None:
        obj.cleanup()


class SuperSloMo(object):
    """Super SloMo class (MI355X implementation of v2ecore.slomo.SuperSloMo)."""
    # The AVI writers (built on first need in interpolate(): the frame size is known there), their frame counts and cv2, here
    # because cleanup() reads them and __del__ calls it on an instance whose constructor raised, too
    ori_writer = slomo_writer = vid_orig = vid_slomo = _cv2 = None
    numOrigVideoFramesWritten = numSlomoVideoFramesWritten = 0
    preview = False

    def __init__(self, model, auto_upsample, upsampling_factor, batch_size=1, video_path=None,
                 vid_orig='original.avi', vid_slomo='slomo.avi', preview=False, avi_frame_rate=30):
        if torch.cuda.is_available():
            self.device = "cuda:0"  # slomo.py:84
        else:
            self.device = "cpu"
            logger.warning('no ROCm GPU visible: v2e_amd.SuperSloMo cannot interpolate (no CPU fallback)')
        self.checkpoint = model
        self.batch_size = batch_size
        if not auto_upsample and (not isinstance(upsampling_factor, int) or upsampling_factor < 2):
            raise ValueError('upsampling_factor={} but must be an int value>1 when auto_upsample=True'.format(
                upsampling_factor))  # slomo.py:91-94
        self.upsampling_factor = upsampling_factor
        self.auto_upsample = auto_upsample
        # slomo.py:110-121: kept as given
        self.video_path = video_path
        self.preview = preview
        self.preview_resized = False
        self.vid_orig, self.vid_slomo, self.avi_frame_rate = vid_orig, vid_slomo, avi_frame_rate
        self._host_video_warned = False
        self.model_loaded = False
        self.engine = None
        self._selfcheck_pending = False  # set by _load_model: the first batch of a loaded checkpoint is checked
        self.mean = 0.428  # slomo.py:148: Normalize(mean=[0.428], std=[1]) on the GPU path only
        # (slomo.py:124 registers cleanup with atexit; through a weak reference: a bound method would keep the instance, its engine and
        #  their device memory alive until the process ends)
        atexit.register(_cleanup_at_exit, weakref.ref(self))

    def __del__(self):
        try:
            self.cleanup()
        except Exception:
            pass

    def cleanup(self):  # slomo.py:126-138
        for w, name, n in ((self.ori_writer, self.vid_orig, self.numOrigVideoFramesWritten),
                           (self.slomo_writer, self.vid_slomo, self.numSlomoVideoFramesWritten)):
            if w is not None:
                logger.info('closing video AVI {} after writing {} frames'.format(name, n))
                try:
                    w.release()
                except Exception:
                    pass
        self.ori_writer = self.slomo_writer = None
        if self.preview and self._cv2 is not None:
            try:
                self._cv2.destroyAllWindows()
            except Exception:
                pass

    def _host_video(self):
        """cv2 for the AVI / preview side outputs (host work, not the hot path), or None with one warning."""
        if self._cv2 is not None:
            return self._cv2
        try:
            import cv2
            if not callable(getattr(cv2, "VideoWriter", None)) or not callable(getattr(cv2, "VideoWriter_fourcc", None)):
                raise ImportError("cv2 has no VideoWriter")
            self._cv2 = cv2
        except Exception as e:
            if not self._host_video_warned:
                logger.warning("v2e_amd.SuperSloMo: video_path=%r / preview=%r need OpenCV on the host (%s): the AVI / preview "
                               "side outputs are skipped, the interpolated frames are written as usual",
                               self.video_path, self.preview, e)
                self._host_video_warned = True
        return self._cv2

    def _open_writers(self, ori_dim):
        """slomo.py:287-301: the AVI writers, now that the frame size is known (v2e_utils.video_writer: codec
        OUTPUT_VIDEO_CODEC_FOURCC, frame size (width, height))."""
        if self.video_path is None or (self.vid_orig is None and self.vid_slomo is None):
            return
        cv2 = self._host_video()
        if cv2 is None:
            return
        fourcc = cv2.VideoWriter_fourcc(*OUTPUT_VIDEO_CODEC_FOURCC)
        size = (int(ori_dim[0]), int(ori_dim[1]))  # frame_size is (width, height), as cv2.VideoWriter wants it
        if self.vid_orig is not None and self.ori_writer is None:
            self.ori_writer = cv2.VideoWriter(os.path.join(self.video_path, self.vid_orig), fourcc, self.avi_frame_rate, size)
        if self.vid_slomo is not None and self.slomo_writer is None:
            self.slomo_writer = cv2.VideoWriter(os.path.join(self.video_path, self.vid_slomo), fourcc, self.avi_frame_rate, size)

    def _write_videos(self, source_frame_path, output_folder):
        """slomo.py:463-490: the source frames and the interpolated PNGs, grey -> 3 equal channels, into the two AVIs."""
        from PIL import Image
        if self.ori_writer is not None:
            for f in sorted(glob.glob("{}".format(source_frame_path) + "/*.npy")):
                a = np.load(f)
                if a.ndim == 2:
                    a = np.repeat(a[:, :, None], 3, axis=2)  # cv2.COLOR_GRAY2BGR
                self.ori_writer.write(np.ascontiguousarray(a))
                self.numOrigVideoFramesWritten += 1
        if self.slomo_writer is not None:
            for f in _all_images(output_folder):
                a = np.asarray(Image.open(f).convert("L"))
                self.slomo_writer.write(np.ascontiguousarray(np.repeat(a[:, :, None], 3, axis=2)))
                self.numSlomoVideoFramesWritten += 1

    def _preview_batch(self, output_folder, first, last):
        """slomo.py:451-468: show the frames just written (needs a display and cv2; off with one warning otherwise)."""
        cv2 = self._host_video()
        if cv2 is None or not callable(getattr(cv2, "imshow", None)):
            return
        try:
            name = "v2e_amd.slomo"
            cv2.namedWindow(name, cv2.WINDOW_NORMAL)
            for idx in range(first, last):
                frame = cv2.imread(os.path.join(output_folder, str(idx) + ".png"))
                cv2.imshow(name, frame)
                if not self.preview_resized:
                    cv2.resizeWindow(name, 800, 600)
                    self.preview_resized = True
                k = cv2.waitKey(1)
                if k == 27 or k == ord('x'):
                    raise SystemExit(0)  # v2e_quit()
        except SystemExit:
            raise
        except Exception as e:  # no display: the side output is dropped
            logger.warning("v2e_amd.SuperSloMo: preview not available (%s)", e)
            self.preview = False

    def _load_model(self):
        if not os.path.isfile(self.checkpoint):
            raise FileNotFoundError('SuperSloMo model checkpoint ' + str(self.checkpoint) +
                                    ' does not exist or is not readable')  # slomo.py:203-205
        logger.info('loading SuperSloMo model from ' + str(self.checkpoint))
        d = torch.load(self.checkpoint, map_location="cpu", weights_only=False)
        self.engine = SloMoEngine(d['state_dictFC'], d['state_dictAT'], self.device)  # slomo.py:225-227
        self.model_loaded = True
        self._selfcheck_pending = os.environ.get("V2E_AMD_SLOMO_SELFCHECK", "1") != "0"

    SELFCHECK_TOLERANCE = 1e-5  # the tolerance the drop-in promises against the reference's float32 arithmetic
    SELFCHECK_WORSE_THAN_EXACT = 2.0  # ... and how much further from the float32 kernels than the exact split 'auto' may be beyond it

    def _first_batch_selfcheck(self, I0, I1):
        """Once per loaded checkpoint, on the first two pairs that come in: the default conv math ('auto': two float16 pieces) against
        the float32-MFMA kernels, in units of each tensor's scale.  Within 1e-5: done.  Above: the exact split ('bf16x3') is measured
        the same way -- on weights with large heads (visibility logits to 100) two float32 summation orders differ by a few 1e-5 in
        the blended frames whatever the operands carry -- and 'auto' is kept if it is no more than 2x further from the float32
        kernels than the exact split; otherwise the engine is rebuilt with the exact split, with one warning.
        V2E_AMD_SLOMO_SELFCHECK=0 skips all this; `python -m v2e_amd.check_ckpt <ckpt>` prints the per-layer picture."""
        self._selfcheck_pending = False
        eng = self.engine
        if eng.conv_math != "auto":
            return
        ref = SloMoEngine(eng._state_dicts[0], eng._state_dicts[1], self.device, conv_math="f32")
        r = eng.self_check(I0[:2], I1[:2], reference=ref)
        self.selfcheck_result = r
        if r["max"] <= self.SELFCHECK_TOLERANCE:
            return
        exact = SloMoEngine(eng._state_dicts[0], eng._state_dicts[1], self.device, conv_math="bf16x3")
        rx = exact.self_check(I0[:2], I1[:2], reference=ref)
        r["exact_split_max"] = rx["max"]
        if r["max"] <= self.SELFCHECK_WORSE_THAN_EXACT * rx["max"]:  # (a NaN fails)
            logger.info("v2e_amd.SuperSloMo: default conv math %.2e from the float32 kernels on the first batch (of the tensors' scale); "
                        "the exact split is %.2e from them: float32 summation order, not operand precision -- keeping the default",
                        r["max"], rx["max"])
            return
        logger.warning("v2e_amd.SuperSloMo: with this checkpoint the default conv math differs from the float32 kernels by %.2e of the "
                       "tensors' scale (flow %.2e, interpolation net %.2e, frames %.2e) on the first batch -- above %.0e and %.1fx what "
                       "the exact split shows (%.2e): switching to the exact three-piece split (conv_math='bf16x3', ~0.7x the frames "
                       "per second)", r["max"], r["flow"], r["intrp"], r["Ft"], self.SELFCHECK_TOLERANCE, r["max"] / max(rx["max"], 1e-30),
                       rx["max"])
        self.engine = exact

    @staticmethod
    def _load_pair_tensor(files, idx, dim):
        """dataloader.py:136-147: np.load -> PIL LANCZOS resize -> ToTensor ([1,H,W] float32 in 0..1)."""
        from PIL import Image
        out = []
        for f in (files[idx], files[idx + 1]):
            img = Image.fromarray(np.load(f)).resize(dim, Image.LANCZOS)
            a = np.asarray(img)
            if a.ndim == 2:
                a = a[None]
            else:
                a = np.transpose(a, (2, 0, 1))
            out.append(torch.from_numpy(a.astype(np.float32) / 255.0))  # ToTensor on uint8
        return out

    def _load_batch(self, files, b0, dim):
        """(I0, I1) of the batch of source pairs from b0 on: normalised [B,1,h,w] float32 on the device."""
        dev = self.engine.device
        pairs = [self._load_pair_tensor(files, i, dim) for i in range(b0, min(b0 + self.batch_size, len(files) - 1))]
        return ((torch.stack([p[0] for p in pairs]) - self.mean).to(dev).contiguous(),
                (torch.stack([p[1] for p in pairs]) - self.mean).to(dev).contiguous())

    def _source_files(self, source_frame_path, output_folder):
        """slomo.py:231-280: the clip's .npy frames in order, once the arguments, the device and the number of batches are in
        order (a batch_size too large for two batches is halved, with a warning, as the reference does)."""
        if not output_folder:
            raise ValueError('output_folder is None; it must be supplied to store the interpolated frames')
        _capi.require_gpu("SuperSloMo", self.device != "cpu")
        nframes = len(os.listdir(source_frame_path))
        if nframes / self.batch_size < 2:
            logger.warning(f'only {nframes} input frames with batch_size={self.batch_size}, automatically '
                           f'reducing batch size to provide at least 2 batches')
            while nframes / self.batch_size < 2:
                self.batch_size = int(self.batch_size / 2)
        files = sorted(glob.glob("{}".format(source_frame_path) + "/*.npy"))  # dataloader.py:115
        nbatches = (len(files) - 1 + self.batch_size - 1) // self.batch_size
        if nbatches < 2:
            raise Exception('there are only {} batches in {} and we need at least 2; maybe you need to reduce batch '
                            'size or increase number of input frames'.format(nbatches, source_frame_path))
        return files

    def _write_batch(self, Ft, output_folder, ori_dim, first):
        """A batch's frames Ft [U,B,1,h,w] as <idx>.png, idx = first + U * pair + k (slomo.py:436-444)."""
        from PIL import Image
        U, B = int(Ft.shape[0]), int(Ft.shape[1])
        dev = self.engine.device
        # ToPILImage after revNormalize (slomo.py:153-161, 437): (x + mean) * 255 -> byte, the CPU conversion the
        # reference performs (truncation, low byte): same kernel as the PNG-free pipeline uses
        q = torch.empty(tuple(Ft.shape), dtype=torch.uint8, device=dev)
        check(self.engine.lib.v2e_f32_to_u8_trunc(ptr(Ft.contiguous()), ptr(q), U, B, int(Ft.shape[-1] * Ft.shape[-2]),
                                                  float(self.mean), 0, stream_ptr(dev)), "v2e_f32_to_u8_trunc")
        img_u8 = q.cpu().numpy()
        for k in range(U):
            for batchIndex in range(B):
                img = Image.fromarray(img_u8[k, batchIndex, 0], mode="L")
                img.resize(ori_dim, Image.BILINEAR).save(os.path.join(output_folder, str(first + U * batchIndex + k) + ".png"))

    def interpolate(self, source_frame_path, output_folder, frame_size):
        """Run interpolation; writes <idx>.png into output_folder (slomo.py:231-495)."""
        files = self._source_files(source_frame_path, output_folder)
        dim = (int(frame_size[0] / 32) * 32, int(frame_size[1] / 32) * 32)  # dataloader.py:122-123
        if not self.model_loaded:
            self._load_model()
        self._open_writers(frame_size)
        outputFrameCounter = inputFrameCounter = 0
        factors, interpTimes = [], []
        starts = list(range(0, len(files) - 1, self.batch_size))
        nxt = self._load_batch(files, starts[0], dim)
        for bi, b0 in enumerate(starts):
            # the next batch is loaded first: its flow UNet runs beside this batch's interpolation UNet (SloMoEngine.flow_ahead)
            I0, I1 = nxt
            nxt = self._load_batch(files, starts[bi + 1], dim) if bi + 1 < len(starts) else None
            if self._selfcheck_pending:
                self._first_batch_selfcheck(I0, I1)
            num_batch_frames = I0.shape[0]
            flowOut = self.engine.flow(I0, I1)
            if self.auto_upsample:  # slomo.py:352-379
                upsampling_factor = factor_from_speed(self.engine.max_speed(flowOut), self.upsampling_factor)
            else:
                upsampling_factor = max(2, self.upsampling_factor)
            factors.append(upsampling_factor)
            interpTimes.append(_batch_interp_times(inputFrameCounter, upsampling_factor, num_batch_frames))
            Ft = self.engine.interpolate(I0, I1, time_points(upsampling_factor), flow=flowOut, next_pair=nxt)  # [U,B,1,H,W]
            self._write_batch(Ft, output_folder, frame_size, outputFrameCounter)
            numOutputFramesThisBatch = upsampling_factor * num_batch_frames
            if self.preview:
                self._preview_batch(output_folder, outputFrameCounter, outputFrameCounter + numOutputFramesThisBatch)
            inputFrameCounter += num_batch_frames
            outputFrameCounter += numOutputFramesThisBatch
        self._write_videos(source_frame_path, output_folder)
        return np.concatenate(interpTimes), sum(factors) / len(factors)

    def get_interpolated_timestamps(self, ts):  # slomo.py:540-564
        new_ts = []
        for i in range(ts.shape[0] - 1):
            start, end = ts[i], ts[i + 1]
            interpolated_ts = np.linspace(start, end, self.upsampling_factor, endpoint=False) + \
                0.5 * (end - start) / self.upsampling_factor
            new_ts.append(interpolated_ts)
        return np.hstack(new_ts)
