"""magic_amd: MI355X-native (gfx950) implementation of VLN-MAGIC's cross-modal transformer +
MAKD distillation training hot path.  Import as ``magic_amd`` (see /magic_amd.py shim)."""
__version__ = "0.1.0"


def __getattr__(name):
    # lazy: `magic_amd.wrap_model` / `magic_amd.DistributedDataParallel` (host/ddp.py) without importing torch at package import
    if name in ("wrap_model", "DistributedDataParallel", "TorchDDPWrapperError"):
        from .host import ddp
        return getattr(ddp, name)
    # the driver's validation block on the device (host/validate.py): `from magic_amd import validate`
    if name in ("Validator", "validate", "validate_mlm", "validate_mrc", "validate_sap", "validate_cfp", "merge_block"):
        from .host import validate as _validate
        return getattr(_validate, name)
    # the navigator's `--optim` / `--use_lr_sch` on the flat buffers (host/trainer.py): `magic_amd.flat_optimizer('rms', model.store, lr)`
    if name in ("FlatOptimizer", "flat_optimizer", "FlatTorchAdamW"):
        from .host import trainer as _trainer
        return getattr(_trainer, name)
    raise AttributeError(name)
