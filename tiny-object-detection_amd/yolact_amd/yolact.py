"""`Yolact` — mirror of the reference's struct (src/yolact.rs:13-41) over the HIP library."""
import os

import numpy as np

from .capi import COMPAT_STRICT, Engine, TfliteEngine


class Yolact:
    """reference: `pub struct Yolact<'a> { interpreter }` (src/yolact.rs:13-15)."""

    def __init__(self, engine, compat_mode):
        self.interpreter = engine
        self.compat_mode = compat_mode

    @classmethod
    def init(cls, model_path=None, weights=None, seed=1, input_size=224, compat_mode=COMPAT_STRICT, device=0, backbone=50,
             max_batch=2):
        """reference: `Yolact::init()` (src/yolact.rs:17-37), which hard-codes
        "data/FRC_model_edgetpu.tflite". Here:
          * model_path = a non-EdgeTPU .tflite (the reference's data/FRC_model.tflite family: a uint8 or int8
            MobileNetV2-style graph with a uint8 input and a uint8 or float32 output 4) -> the TFLite model path runs it on the GPU, with room for max_batch images per
            invoke (TfliteEngine's max_images; classify_batch on n frames needs 2n);
          * otherwise the YOLACT R50/R101 engine at `input_size` (224 = the reference's tile,
            yolact.rs:143-144) with `weights` (a YHW1 blob) or the seeded synthetic blob; max_batch tiles
            per step (classify_batch on n frames needs 2n).
        Errors raise (the reference `.expect`s every failure)."""
        if model_path is not None:
            if not os.path.exists(model_path):
                raise FileNotFoundError(f"failed to load model: {model_path}")   # yolact.rs:20
            with open(model_path, "rb") as f:
                return cls(TfliteEngine(f.read(), device=device, max_images=max(2, max_batch)), compat_mode)
        eng = Engine(input_size=input_size, backbone=backbone, max_batch=max_batch, use_graph=True, device=device)
        eng.load_weights(weights if weights is not None else eng.generate_weights(seed))
        return cls(eng, compat_mode)

    def classify(self, frame_buffer, width=640, height=480):
        """reference: `classify(&mut self, frame_buffer: &mut [u32])` (src/yolact.rs:39-41, :192-234):
        overwrites the packed camera frame (r<<24|g<<16|b<<8, src/scene.rs:86) in place."""
        assert isinstance(frame_buffer, np.ndarray) and frame_buffer.dtype == np.uint32
        self.interpreter.classify_frame(frame_buffer.reshape(-1), width, height, self.compat_mode)

    def classify_batch(self, frames, width=640, height=480):
        """classify on n frames at once, in place on a uint32 [n][height * width] array: one network step of 2n tiles
        (Engine.classify_batch or TfliteEngine.classify_batch; the handle needs max_batch >= 2n). Returns the per-frame divergence flags (all zero)."""
        assert isinstance(frames, np.ndarray) and frames.dtype == np.uint32 and frames.flags.c_contiguous
        n = frames.size // (width * height)
        _, diverged = self.interpreter.classify_batch(frames_u32=frames, n=n, width=width, height=height, mode=self.compat_mode,
                                                      out=frames)
        return diverged
