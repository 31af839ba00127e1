"""Drop-in package name for the four GAN recommenders this repository implements.

RecSysExp.py decides "isGAN" from `cls.__module__.split('.')[0] == 'GANRec'` (RecSysExp.py:202-204) and imports
`GANRec.GANMF.GANMF` / `GANRec.DisGANMF.DisGANMF` / `GANRec.CFGAN.CFGAN` / `GANRec.CAAE.CAAE` (RecSysExp.py:41-45): all four resolve
here.  With this repository AHEAD of the reference on `sys.path` (option A) this package still does not hide the
reference's: `extend_path` appends every other `GANRec/` directory found on `sys.path` to the package search path, so the four
modules above resolve here (first entry) and any other submodule (the reference's `GANRec.Cython`, say) resolves in the
reference's directory."""
import pkgutil

__path__ = pkgutil.extend_path(__path__, __name__)
