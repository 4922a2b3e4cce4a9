"""The floating-base estimator chain (tests/fb_chain.py) on the CPU stand-in engine against tests/golden/ref_identification_fb.npz, the
committed outputs of the reference's own ``Identification`` on the same files: threeLinks with configs/threeLinks.yaml (data-driven QR,
OLS) and WALK-MAN with the configs/walkman_full.yaml option set (base-wrench rows, trajectory weighting over two files, contact wrenches,
post-identification friction).  What is exercised here is the Model / Data / estimation surface the chain drives, not the kernels; the
same chain on the HIP engine is tests/test_gpu_dropin_fb.py."""
import pytest

import cpu_engine
import fb_chain


@pytest.fixture
def stand_in_model(monkeypatch):
    from flobaroid_amd.model import Model

    def _engine(self):
        if self._engine is None:
            o = self.opt
            self._engine = cpu_engine.NumpyOracleEngine(self.topology, floating=o["floatingBase"], friction=o["identifyFrictionSimultaneously"],
                                                        friction_symmetric=o["identifySymmetricVelFriction"], gravity_only=o["identifyGravityParamsOnly"],
                                                        stribeck_velocity=float(o.get("stribeckVelocity", 0) or 0.0))
        return self._engine

    monkeypatch.setattr(Model, "engine", property(_engine))
    return Model


@pytest.mark.parametrize("name", ["threelinks", "walkman"])
def test_floating_base_chain_on_the_stand_in_engine_matches_the_fixture(stand_in_model, tmp_path, name, capsys):
    from flobaroid_amd.data import Data

    z = fb_chain.load_fixture()
    assert int(z[name + "_out_num_base_params"]) == (24 if name == "threelinks" else 213)
    opt, files, topo, tpath = fb_chain.write_inputs(z, name, tmp_path)
    out = fb_chain.run_chain(opt, files, topo, tpath, stand_in_model, Data)
    fb_chain.compare(out, z, name, 1e-7)
    capsys.readouterr()
