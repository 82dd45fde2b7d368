"""MI355X-native AudioLDM + LoRA hot path (gfx950 HIP kernels behind a C-ABI).

Drop-in surface for the reference's entry points:
AudioLDMPipeline / UNet2DConditionModel / AutoencoderKL / SpeechT5HifiGan / DDIMScheduler / DPMSolverMultistepScheduler /
UniPCMultistepScheduler / EulerAncestralDiscreteScheduler / RePaintScheduler (all five in scheduler.py; the last three exported here on first use as well) and the peft-shaped LoraConfig / get_peft_model helpers; AudioLDMAudioToAudioPipeline (audio2audio.py,
exported here on first use) starts from a recording; Resampler / resample (resample.py, likewise) bring audio of any rate to another
on the device; ClipFrontEnd / HfAudioDataset / AudioFolder / ClipLoader (data.py, likewise) turn recordings into training batches
there.  No CPU fallback: ops raise if libaldm_hip.so is missing.
"""
__version__ = "0.1.0"


def __getattr__(name):
    if name == "AudioLDMAudioToAudioPipeline":
        from .audio2audio import AudioLDMAudioToAudioPipeline
        return AudioLDMAudioToAudioPipeline
    if name == "UniPCMultistepScheduler":
        from .scheduler import UniPCMultistepScheduler
        return UniPCMultistepScheduler
    if name == "EulerAncestralDiscreteScheduler":
        from .scheduler import EulerAncestralDiscreteScheduler
        return EulerAncestralDiscreteScheduler
    if name == "RePaintScheduler":
        from .scheduler import RePaintScheduler
        return RePaintScheduler
    if name == "Resampler":
        from .resample import Resampler
        return Resampler
    if name == "resample":                              # the function; resample.py makes its module callable as it (and keeps the name)
        import importlib
        return importlib.import_module(".resample", __name__)
    if name in ("LoudnessMeter", "integrated_loudness", "normalize_loudness"):       # loudness.py: BS.1770 metering and normalisation
        from . import loudness
        return getattr(loudness, name)
    if name in ("ClipFrontEnd", "HfAudioDataset", "AudioFolder", "ClipLoader", "ByteTokenizer"):      # data.py: training from recordings
        from . import data
        return getattr(data, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
