"""
_golden_models.py — the models and reference configurations of the ved_*, vedbn_* and ivaeconv_* fixtures, built from a
fixture's meta as tests/golden/make_golden.py built them.
"""
import ast

from conftest import meta_of

import pyroved_amd as pv
from oracle import svi_oracle as orc


def ved_case(gold):
    kw = {}
    for k in gold:
        if k.startswith("meta.model_kw."):
            v = str(gold[k])
            kw[k[len("meta.model_kw."):]] = ast.literal_eval(v) if (v[0] in "[(" or v in ("True", "False")) else v
    return dict(input_dim=tuple(int(v) for v in gold["meta.input_dim"]),
                output_dim=tuple(int(v) for v in gold["meta.output_dim"]),
                latent_dim=int(gold["meta.latent_dim"]), steps=int(gold["meta.steps"]),
                beta=float(gold["meta.scale_factor"]), kw=kw)


def vedbn_oracle(gold, device="cpu"):
    c = ved_case(gold)
    model = pv.models.VED(c["input_dim"], c["output_dim"], latent_dim=c["latent_dim"], seed=1, device=device, **c["kw"])
    cfg = orc.VedConfig(input_dim=c["input_dim"], output_dim=c["output_dim"], latent_dim=c["latent_dim"],
                        hidden_dim_e=c["kw"].get("hidden_dim_e"), hidden_dim_d=c["kw"].get("hidden_dim_d"),
                        activation=c["kw"].get("activation", "lrelu"), batchnorm=True)
    return c, model, cfg


def convenc_model(gold, device):
    """iVAE + set_encoder(convEncoderNet(data_dim, latent_dim=z_dim, hidden_dim=...)) built like the fixture's model."""
    meta = meta_of(gold)
    hid = ast.literal_eval(str(gold["meta.conv_encoder"]))
    model = pv.models.iVAE(meta["data_dim"], meta["latent_dim"], meta["invariances"], seed=1, device=device)
    model.set_encoder(pv.nets.convEncoderNet(meta["data_dim"], latent_dim=model.z_dim, hidden_dim=hid))
    cfg = orc.Config(data_dim=meta["data_dim"], latent_dim=meta["latent_dim"], invariances=meta["invariances"],
                     conv_encoder=hid)
    return meta, model, cfg
