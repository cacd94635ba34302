"""Model classes for the sibling heads: the reference's `MODEL(...)`, `.compile(...)`, `.fit(...)`, `.predict(...)`,
`.evaluate(...)` (models/basemodel.py, models/mtl_basemodel.py) over the modules of layers.py.

    model = WDL(linear_feature_columns, dnn_feature_columns, seed=seed, device="cuda:0", domain_column=col, num_domains=n, flag=flag)
    model.compile(torch.optim.Adam(model.parameters(), lr), "binary_crossentropy", metrics=["binary_crossentropy", "auc"])
    model.fit(x=train_input, y=labels, batch_size=8192, epochs=1, verbose=1)
    pred = model.predict(test_input, 4 * 8192)

`HeadModel` is not a subclass of this package's `BaseModel` (the SATrans engine); it borrows that class's input packing and its
readers of compile()'s arguments.  A model is `FeatureEmbedding(dnn_feature_columns)`, `LinearModel(linear_feature_columns)` and a
head.  One training step is: forward; `PointLoss` (prediction, summed loss and its gradient in one launch); total = loss +
head.regularization_loss() + aux_loss; backward; `TableAdam.step()` for the tables and `torch.optim.Adam.step()` for the head.
The step totals are added on the device in double; the harness itself reads nothing back inside an epoch with verbose=0 (the lookup
modules and the scenario heads each keep their one status / bucket read per forward).  At epoch end the tables are flushed and
History["loss"] = (sum of the step totals + the tables' regulariser total of the epoch) / sample_num (basemodel.py:353).

state_dict() carries the reference's keys in the reference's order (`embedding_dict.*`, `linear_model.*`, `out.bias`, the head's
own), so a reference checkpoint loads; entries of the reference's unused meta modules (`domain_embeddings.*`, `domain_map_dnn.*`,
`meta_net.*`, created whenever `domain_column` is given) are skipped on load and absent on save.

Built: every non-SATrans branch of main.py:211-281 - WDL, DCN, DeepFM, xDeepFM, NFM, AutoInt, AFM, FiBiNET, PNN, AdaSparse;
SharedBottom, MMOE, PLE, ESMM; Star_Net (as main.py builds it: use_domain_dnn=True, domain_id_as_feature=True).  ESMM's head ends
in two probabilities, not one logit: it replaces `_loss_and_pred` and takes its loss by RoutedPointLoss.  Not built: a `flag`
containing metatrans / usemetatrans / usetrans / nofm / nodnn, valid_cnt_per_epoch > 1, `gpus`, bf16, sample weights, unequal
per-task losses."""
from __future__ import annotations

import time
import warnings
from collections import OrderedDict

import numpy as np
import torch
import torch.nn as nn

from . import device_metrics as DM
from .basemodel import BaseModel
from .callbacks import CallbackList, History
from .inputs import PackedInput, build_input_features
from .layers import (AdaSparseHead, AFMHead, AutoIntHead, DCNHead, DeepFMHead, ESMMHead, FeatureEmbedding, FiBiNETHead, LinearModel,
                     MMoEHead, NFMHead, PLEHead, PNNHead, PointLoss, RoutedPointLoss, SharedBottomHead, StarHead, WDLHead, XDeepFMHead,
                     _OutBias)
from .optim import TableAdam

_META_PREFIXES = ("domain_embeddings.", "domain_map_dnn.", "meta_net.")
_TORCH_OPTIMIZERS = {"sgd": (torch.optim.SGD, dict(lr=0.01)), "adagrad": (torch.optim.Adagrad, dict(lr=0.01)),
                     "rmsprop": (torch.optim.RMSprop, dict(lr=0.01))}


def _refuse_flag(flag, words):
    for word in words:
        if flag and word in flag:
            raise NotImplementedError(f"flag {flag!r}: {word} is not built for this model")


class HeadModel(nn.Module):
    """See the module docstring.  Subclasses set `self.head` (and call `_finish()`), and implement `_logit(X)` -> [B, 1] (or
    replace `_loss_and_pred`)."""

    # the readers the SATrans BaseModel already has: plain functions of (self, ...) over feature_index / dnn_feature_columns / device
    _pack = BaseModel._pack
    _host_matrices = BaseModel._host_matrices
    _to_device_matrix = BaseModel._to_device_matrix
    _get_metrics = BaseModel._get_metrics
    returns_column = True      # predict -> [n, 1]; the multi-task models return [n]
    num_tasks = 1

    def __init__(self, linear_feature_columns, dnn_feature_columns, l2_reg_linear=1e-5, l2_reg_embedding=1e-5, init_std=0.0001,
                 seed=1024, task='binary', device='cpu', gpus=None, flag=None, domain_column=None, num_domains=None,
                 linear_in_forward=True):
        super().__init__()
        if gpus:
            raise NotImplementedError("gpus: several ranks are not built for the sibling models")
        if task not in ("binary", "regression"):
            raise ValueError("task must be binary or regression")
        _refuse_flag(flag, ("metatrans",))
        torch.manual_seed(seed)
        self.flag, self.task, self.device = flag, task, device
        self.domain_column, self.num_domains = domain_column, num_domains
        self.linear_feature_columns, self.dnn_feature_columns = list(linear_feature_columns), list(dnn_feature_columns)
        self.l2_reg_linear, self.l2_reg_embedding = float(l2_reg_linear), float(l2_reg_embedding)
        self.feature_index = build_input_features(self.linear_feature_columns + self.dnn_feature_columns)
        self.embedding = FeatureEmbedding(self.dnn_feature_columns, self.feature_index, init_std, device)
        self.linear_model = LinearModel(self.linear_feature_columns, self.feature_index, init_std, device)
        # (wdl.py, mmoe.py and star.py leave linear_model out of the logit: its parameters then see the regulariser alone)
        self._linear_in_forward = bool(linear_in_forward) and any(True for _ in self.linear_model.parameters())
        self.aux_loss = torch.zeros((1,), device=device)
        self.domain_id_offset = 0
        self.history = History()
        self.stop_training = False
        self._table_opt = self._dense_opt = None
        self._all_torch = False
        self._point = PointLoss("binary_crossentropy", task)

    def _finish(self):
        self.to(self.device)

    # ---- forward -----------------------------------------------------------------------------------------------------------------
    def _inputs(self, X):
        emb, dense = self.embedding(X)
        return emb, dense

    def _dnn_input(self, X):
        emb, dense = self._inputs(X)
        flat = emb.flatten(1)
        return flat if dense is None else torch.cat([flat, dense], dim=1)

    def _domain_ids(self, X):
        ids = X.ids if isinstance(X, PackedInput) else X
        return ids[:, self.feature_index[self.domain_column][0]]

    def _logit(self, X):
        raise NotImplementedError

    def _loss_and_pred(self, X, y=None):
        """The tail of the forward, which train_step and forward both go through -> (loss sum or None, pred [B, 1]).  A model
        whose head does not end in one logit column (ESMM) replaces it."""
        return self._point(self._logit(X), y)

    def forward(self, X):
        """The reference's forward: the prediction [B, 1] (the multi-task models: each row's own task)."""
        return self._loss_and_pred(X)[1]

    def regularization_loss(self):
        """What the torch side of the step adds to the loss: the head's own regulariser, and that of a linear_model outside the
        logit or of every table when no TableAdam steps them."""
        total = torch.zeros((1,), device=self.aux_loss.device)
        if hasattr(self.head, "regularization_loss"):
            total = total + self.head.regularization_loss()
        groups = []
        if self._all_torch:
            groups.append((self.embedding.parameters(), self.l2_reg_embedding))
        if self._all_torch or not self._linear_in_forward:
            groups.append((self.linear_model.parameters(), self.l2_reg_linear))
        for params, l2 in groups:
            if l2 > 0:
                for p in params:
                    total = total + torch.sum(l2 * torch.square(p))
        return total

    # ---- state -------------------------------------------------------------------------------------------------------------------
    def state_dict(self, *args, **kwargs):
        sd = super().state_dict(*args, **kwargs)
        prefix = kwargs.get("prefix", "")
        out = OrderedDict()
        for k, v in sd.items():
            body = k[len(prefix):]
            for inner in ("embedding.", "head."):
                if body.startswith(inner):
                    body = body[len(inner):]
                    break
            out[prefix + body] = v
        if hasattr(sd, "_metadata"):
            out._metadata = sd._metadata
        return out

    def load_state_dict(self, state_dict, strict=True, **kwargs):
        if self._table_opt is not None:
            self._table_opt.flush()
        mapped = OrderedDict()
        own_out = "out" in self._modules
        for k, v in state_dict.items():
            if k.startswith(_META_PREFIXES):
                continue
            if k.startswith("embedding_dict."):
                k = "embedding." + k
            elif not (k.startswith("linear_model.") or (own_out and k.startswith("out."))):
                k = "head." + k
            mapped[k] = v
        return super().load_state_dict(mapped, strict=strict, **kwargs)

    # ---- compile -----------------------------------------------------------------------------------------------------------------
    def compile(self, optimizer, loss=None, metrics=None):
        """Arguments as the reference's (basemodel.py / mtl_basemodel.py `compile`).  Adam - an instance over model.parameters() or
        "adam" - is read for lr / betas / eps: the tables step by TableAdam(track_regularizer=True), the head by a torch.optim.Adam
        with the same constants.  SGD / Adagrad / RMSprop: the optimizer is rebuilt over all parameters with dense gradients (the
        slow route of the un-adopted modules), with a warning.  `loss`: a name, or num_tasks equal names."""
        self.metrics_names = ["loss"]
        cfg = BaseModel._read_optimizer(optimizer)
        if isinstance(loss, (list, tuple)):
            if len(loss) != self.num_tasks:
                raise ValueError("the length of `loss` should be equal with `self.num_tasks`")
            if len(set(loss)) != 1:
                raise NotImplementedError(f"a list of unequal losses {list(loss)}: every task takes the same loss")
            loss = loss[0]
        self.loss_func = BaseModel._get_loss_func(loss)
        self.metrics = self._get_metrics(metrics)
        self._point = PointLoss(self.loss_func, self.task)
        self.optim = optimizer
        if self._table_opt is not None:          # compiled again: the earlier optimizer lets go of the tables
            self._table_opt.flush()
            for rec in self._table_opt._adopted:
                rec.mod._table_opt = None
        self._table_opt, self._all_torch = None, cfg["kind"] != "adam"
        if self._all_torch:
            warnings.warn(f"{type(self).__name__}.compile: {cfg['kind']} steps every table through dense gradients (the slow route); "
                          f"only Adam has the touched-rows step")
            if isinstance(optimizer, str):
                cls, defaults = _TORCH_OPTIMIZERS[optimizer]
            else:
                cls, defaults = type(optimizer), {k: v for k, v in optimizer.defaults.items()}
            self._dense_opt = cls(list(self.parameters()), **defaults)
            return
        tables = [self.embedding] + ([self.linear_model] if self._linear_in_forward else [])
        hyper = dict(lr=cfg["lr"], betas=cfg["betas"], eps=cfg["eps"])
        self._table_opt = TableAdam(tables, l2_reg_embedding=self.l2_reg_embedding, l2_reg_linear=self.l2_reg_linear,
                                    track_regularizer=True, **getattr(self, "_table_adam_options", {}), **hyper)
        taken = {id(p) for mod in tables for p in mod.parameters()}
        self._dense_opt = torch.optim.Adam([p for p in self.parameters() if id(p) not in taken], **hyper)

    def add_auxiliary_loss(self, aux_loss, alpha):
        self.aux_loss = aux_loss * alpha

    # ---- data --------------------------------------------------------------------------------------------------------------------
    def _upload(self, x):
        packed = self._pack(x)
        if self.domain_column is not None and type(self).uses_domains:
            self.domain_id_offset = int(packed[:, self.feature_index[self.domain_column][0]].min())
        return self._to_device_matrix(packed)

    @staticmethod
    def _rows(X, index):
        if isinstance(X, PackedInput):
            return PackedInput(X.ids[index], X.dense[index])
        return X[index]

    @staticmethod
    def _count(X):
        return (X.ids if isinstance(X, PackedInput) else X).shape[0]

    # ---- fit ---------------------------------------------------------------------------------------------------------------------
    def train_step(self, Xb, yb):
        """One step on a device batch -> (the step's total as the torch side sees it: [1] fp64 on the device, pred [B, 1])."""
        loss, pred = self._loss_and_pred(Xb, yb)
        total = loss + self.regularization_loss() + self.aux_loss
        self._dense_opt.zero_grad(set_to_none=True)
        total.backward()
        if self._table_opt is not None:
            self._table_opt.step()
        self._dense_opt.step()
        return total.detach(), pred

    def fit(self, x=None, y=None, batch_size=None, epochs=1, verbose=1, initial_epoch=0, validation_split=0., validation_data=None,
            shuffle=True, callbacks=None, valid_cnt_per_epoch=1):
        """Train; arguments and return value as the reference's fit (basemodel.py:201-384, mtl_basemodel.py:142-329)."""
        if valid_cnt_per_epoch is not None and valid_cnt_per_epoch > 1:
            raise NotImplementedError("valid_cnt_per_epoch > 1 is not built")
        if self._dense_opt is None:
            raise RuntimeError("compile() the model before fit()")
        y = np.asarray(y, dtype=np.float32).reshape(-1)
        do_validation, val_x, val_y = False, None, []
        if validation_data:
            if len(validation_data) not in (2, 3):
                raise ValueError("`validation_data` must be (x_val, y_val) or (x_val, y_val, val_sample_weights); "
                                 "received %s" % (validation_data,))
            do_validation, val_x, val_y = True, validation_data[0], np.asarray(validation_data[1])
        X = self._upload(x)                                # one upload; the batches are device-side slices
        if not validation_data and validation_split and 0. < validation_split < 1.:
            do_validation = True
            split_at = int(self._count(X) * (1. - validation_split))
            val_x, val_y = self._rows(X, slice(split_at, None)), y[split_at:]
            X, y = self._rows(X, slice(0, split_at)), y[:split_at]
        dev = self.aux_loss.device
        yd = torch.from_numpy(np.ascontiguousarray(y)).to(dev)
        batch_size = 256 if batch_size is None else batch_size
        sample_num = self._count(X)
        steps_per_epoch = (sample_num - 1) // batch_size + 1
        fused = torch.zeros(2, dtype=torch.float64, device=dev)

        callbacks = CallbackList((callbacks or []) + [self.history])
        callbacks.set_model(self)
        callbacks.on_train_begin()
        self.stop_training = False
        if verbose:
            print("Train on {0} samples, validate on {1} samples, {2} steps per epoch".format(sample_num, len(val_y), steps_per_epoch))
        for epoch in range(initial_epoch, epochs):
            callbacks.on_epoch_begin(epoch)
            self.train()
            start_time = time.time()
            epoch_total = torch.zeros((), dtype=torch.float64, device=dev)
            if self._table_opt is not None:
                self._table_opt.zero_regularization_sum()
            order = torch.randperm(sample_num).to(dev) if shuffle else None
            train_result = {}
            for step in range(steps_per_epoch):
                lo, hi = step * batch_size, min(sample_num, (step + 1) * batch_size)
                index = order[lo:hi] if shuffle else slice(lo, hi)
                Xb, yb = self._rows(X, index), yd[index]
                total, pred = self.train_step(Xb, yb)
                epoch_total += total.sum()
                if verbose > 0 and self.metrics:
                    names = list(self.metrics)
                    if DM.fused_supported(names, hi - lo, yb, pred):
                        DM.fused_logloss_auc(yb, pred, fused)
                        vals = {k: fused[1 if k == "auc" else 0].clone() for k in names}
                    else:
                        vals = {k: DM.BY_NAME[k](yb, pred.reshape(-1)) for k in names}
                    for k, v in vals.items():
                        train_result.setdefault(k, []).append(v)
            if self._table_opt is not None:
                self._table_opt.flush()
                epoch_total = epoch_total + self._table_opt.regularization_sum()
            epoch_logs = {"loss": float(epoch_total.item()) / sample_num}      # the epoch's one read of the loss
            for name, vals in train_result.items():
                epoch_logs[name] = float(torch.stack([v.double() for v in vals]).sum().item()) / steps_per_epoch
            if do_validation:
                offset = self.domain_id_offset            # (the reference's fit keeps the `bias` of its own x)
                for name, result in self.evaluate(val_x, val_y, batch_size).items():
                    epoch_logs["val_" + name] = result
                self.domain_id_offset = offset
            if verbose > 0:
                line = "Epoch {0}/{1}\n{2}s - loss: {3: .4f}".format(epoch + 1, epochs, int(time.time() - start_time), epoch_logs["loss"])
                for name in self.metrics:
                    line += " - " + name + ": {0: .4f}".format(epoch_logs[name])
                    if do_validation:
                        line += " - val_" + name + ": {0: .4f}".format(epoch_logs["val_" + name])
                print(line)
            callbacks.on_epoch_end(epoch, epoch_logs)
            if self.stop_training:
                break
        callbacks.on_train_end()
        return self.history

    # ---- predict / evaluate ------------------------------------------------------------------------------------------------------
    def _predict_device(self, x, batch_size=256):
        """-> pred [n] fp32 on the device (eval mode, no_grad; the adopted forward replays postponed rows itself)."""
        X = x if torch.is_tensor(x) or isinstance(x, PackedInput) else self._upload(x)
        self.eval()
        n, out = self._count(X), []
        with torch.no_grad():
            for lo in range(0, n, batch_size):
                out.append(self.forward(self._rows(X, slice(lo, min(n, lo + batch_size)))).reshape(-1))
        return torch.cat(out)

    def predict(self, x, batch_size=256):
        """float64 probabilities: [n, 1] (basemodel.py:400-459), the multi-task models [n] (mtl_basemodel.py:345-383)."""
        pred = self._predict_device(x, batch_size).cpu().numpy().astype("float64")
        return pred.reshape(-1, 1) if self.returns_column else pred

    def evaluate(self, x, y, batch_size=256):
        """Metric name -> value on (x, y), computed on the device (device_metrics, equal to sklearn's)."""
        pred = self._predict_device(x, batch_size)
        yd = torch.as_tensor(np.asarray(y, dtype=np.float32).reshape(-1)).to(pred.device)
        return {name: float(DM.BY_NAME[name](yd, pred)) for name in self.metrics}

    def evaluate_domains(self, x, y, batch_size=256, domain_col=None):
        """The test report of main.py:353-374: -> {"auc", "domain_auc": {id: auc}, "loss", "pred"} (as BaseModel.evaluate_domains)."""
        domain_col = self.domain_column if domain_col is None else domain_col
        pred = self._predict_device(x, batch_size)
        ids = x[domain_col] if isinstance(x, dict) else self._pack(x)[:, self.feature_index[domain_col][0]]
        dev = pred.device
        auc, per, loss = DM.per_domain_auc(torch.as_tensor(np.asarray(y, dtype=np.float64).reshape(-1)).to(dev), pred.double(),
                                           torch.as_tensor(np.asarray(ids).astype(np.int64).reshape(-1)).to(dev))
        out = pred.cpu().numpy().astype("float64")
        return {"auc": auc, "domain_auc": per, "loss": loss, "pred": out.reshape(-1, 1) if self.returns_column else out}

    uses_domains = False


def _dense_dim(columns):
    from .inputs import split_columns
    return sum(c.dimension for c in split_columns(columns)[1])


def _field_count(columns):
    from .inputs import split_columns
    sparse, _, varlen = split_columns(columns)
    return len(sparse) + len(varlen)


class WDL(HeadModel):
    """models/wdl.py: logit = dnn_linear(dnn(dnn_input)); `linear_model` exists, is regularised and trained, and stays out of the
    logit, as in the reference.  dnn_dropout is WDLHead's (the kernels' own masks)."""

    def __init__(self, linear_feature_columns, dnn_feature_columns, dnn_hidden_units=(256, 128), l2_reg_linear=1e-5,
                 l2_reg_embedding=1e-5, l2_reg_dnn=0, init_std=0.0001, seed=1024, dnn_dropout=0, dnn_activation='relu',
                 dnn_use_bn=False, task='binary', device='cpu', gpus=None, flag=None, domain_column=None, num_domains=None):
        super().__init__(linear_feature_columns, dnn_feature_columns, l2_reg_linear, l2_reg_embedding, init_std, seed, task, device,
                         gpus, flag, domain_column, num_domains, linear_in_forward=False)
        inputs_dim = _field_count(dnn_feature_columns) * self.embedding.embedding_size + _dense_dim(dnn_feature_columns)
        self.head = WDLHead(inputs_dim, dnn_hidden_units, l2_reg_dnn, init_std, dnn_dropout, dnn_activation, dnn_use_bn)
        self._finish()

    def _logit(self, X):
        return self.head(self._dnn_input(X))


class DeepFM(HeadModel):
    """models/deepfm.py: logit = linear_model(X) + FM(emb) + dnn_linear(dnn(dnn_input))."""

    def __init__(self, linear_feature_columns, dnn_feature_columns, use_fm=True, dnn_hidden_units=(256, 128), l2_reg_linear=0.00001,
                 l2_reg_embedding=0.00001, l2_reg_dnn=0, init_std=0.0001, seed=1024, dnn_dropout=0, dnn_activation='relu',
                 dnn_use_bn=False, task='binary', device='cpu', gpus=None, flag=None, domain_column=None, num_domains=None,
                 meta_dnn_hidden_units=(32, 64, 32)):
        _refuse_flag(flag, ("nofm", "nodnn"))
        super().__init__(linear_feature_columns, dnn_feature_columns, l2_reg_linear, l2_reg_embedding, init_std, seed, task, device,
                         gpus, flag, domain_column, num_domains)
        self.head = DeepFMHead(_field_count(dnn_feature_columns), self.embedding.embedding_size, _dense_dim(dnn_feature_columns), use_fm,
                               dnn_hidden_units, l2_reg_dnn, init_std, dnn_dropout, dnn_activation, dnn_use_bn)
        self._finish()

    def _logit(self, X):
        emb, dense = self._inputs(X)
        return self.head(emb, dense, self.linear_model(X))


class DCN(HeadModel):
    """models/dcn.py, vector and matrix form: logit = linear_model(X) + dnn_linear(cat(crossnet(x), dnn(x))).  As in the reference,
    `l2_reg_linear` regularises dnn_linear.weight while linear_model keeps the base class's 1e-5."""

    def __init__(self, linear_feature_columns, dnn_feature_columns, cross_num=2, cross_parameterization='vector',
                 dnn_hidden_units=(128, 128), l2_reg_linear=0.00001, l2_reg_embedding=0.00001, l2_reg_cross=0.00001, l2_reg_dnn=0,
                 init_std=0.0001, seed=1024, dnn_dropout=0, dnn_activation='relu', dnn_use_bn=False, task='binary', device='cpu',
                 gpus=None, flag=None, domain_column=None, num_domains=None, meta_dnn_hidden_units=(32, 64, 32)):
        for name, val, off in (("l2_reg_dnn", l2_reg_dnn, 0), ("dnn_dropout", dnn_dropout, 0), ("dnn_activation", dnn_activation, 'relu'),
                               ("dnn_use_bn", dnn_use_bn, False)):
            if val != off:
                raise NotImplementedError(f"DCNHead: {name}={val!r} is not built")
        super().__init__(linear_feature_columns, dnn_feature_columns, 1e-5, l2_reg_embedding, init_std, seed, task, device, gpus, flag,
                         domain_column, num_domains)
        self.head = DCNHead(_field_count(dnn_feature_columns), self.embedding.embedding_size, _dense_dim(dnn_feature_columns), cross_num,
                            cross_parameterization, dnn_hidden_units, l2_reg_linear, l2_reg_cross, init_std)
        self._finish()

    def _logit(self, X):
        emb, dense = self._inputs(X)
        return self.head(emb, dense, self.linear_model(X))


class _ScenarioModel(HeadModel):
    uses_domains = True

    def _logit(self, X):
        return self.head(self._dnn_input(X), self._domain_ids(X), self.domain_id_offset)


class MMOE(_ScenarioModel):
    """models/mmoe.py behind models/mtl_basemodel.py, one task per scenario: MMoEHead returns each row's own task logit, so the
    reference's masked per-task loss sum (mtl_basemodel.py:268-269) and its per-task predict assembly (:376-378) are PointLoss
    and its `pred` as they are.  predict -> [n].  `domain_id_offset` is the scenario column's minimum over the x of the call."""
    returns_column = False

    def __init__(self, dnn_feature_columns, num_experts=3, expert_dnn_hidden_units=(256, 128), gate_dnn_hidden_units=(64,),
                 tower_dnn_hidden_units=(64,), l2_reg_linear=0.00001, l2_reg_embedding=0.00001, l2_reg_dnn=0, init_std=0.0001,
                 seed=1024, dnn_dropout=0, dnn_activation='relu', dnn_use_bn=False, task_types=('binary', 'binary'),
                 task_names=('ctr', 'ctcvr'), device='cpu', gpus=None, domain_column=None, flag=None):
        _refuse_flag(flag, ("usetrans",))
        if len(task_types) != len(task_names):
            raise ValueError("num_tasks must be equal to the length of task_types")
        for task_type in task_types:
            if task_type not in ('binary', 'regression'):
                raise ValueError("task must be binary or regression, {} is illegal".format(task_type))
        if len(set(task_types)) > 1:
            raise NotImplementedError(f"task_types {list(task_types)}: every task takes the same type")
        if l2_reg_dnn != 0:
            raise NotImplementedError("MMoEHead: l2_reg_dnn is not applied (it must be 0)")
        if domain_column is None:
            raise ValueError("MMOE: domain_column names the column whose id picks a row's task")
        super().__init__([], dnn_feature_columns, l2_reg_linear, l2_reg_embedding, init_std, seed, task_types[0] if task_types else 'binary',
                         device, gpus, flag, domain_column, len(task_names), linear_in_forward=False)
        self.num_tasks, self.task_names = len(task_names), tuple(task_names)
        inputs_dim = _field_count(dnn_feature_columns) * self.embedding.embedding_size + _dense_dim(dnn_feature_columns)
        self.head = MMoEHead(inputs_dim, self.num_tasks, num_experts, expert_dnn_hidden_units, gate_dnn_hidden_units,
                             tower_dnn_hidden_units, init_std, dnn_activation, dnn_dropout, dnn_use_bn)
        self._finish()


class Star_Net(_ScenarioModel):
    """models/star.py as main.py:272-281 builds it (use_domain_dnn=True, domain_id_as_feature=True; use_domain_bn as given):
    StarHead over dnn_input.  `out.bias` exists and stays unused, as in the reference, whose linear_model (l2 0) is unused too."""

    def __init__(self, linear_feature_columns, dnn_feature_columns, domain_column, num_domains, domain_id_as_feature=False,
                 att_layer_num=3, dnn_hidden_units=(256, 128), use_domain_dnn=False, use_domain_bn=False, dnn_activation='relu',
                 l2_reg_dnn=0, l2_reg_embedding=1e-5, dnn_use_bn=False, dnn_dropout=0, init_std=0.0001, seed=1024, task='binary',
                 device='cpu', gpus=None, flag=None):
        _refuse_flag(flag, ("usetrans",))
        if not use_domain_dnn:
            raise NotImplementedError("Star_Net: use_domain_dnn=False (one plain DNN) is not built; main.py passes True")
        if not domain_id_as_feature:
            raise NotImplementedError("Star_Net: domain_id_as_feature=False is not built; main.py passes True")
        if task != 'binary':
            raise NotImplementedError("Star_Net: the towers end in a sigmoid (task must be binary)")
        super().__init__(linear_feature_columns, dnn_feature_columns, 0, l2_reg_embedding, init_std, seed, task, device, gpus, flag,
                         domain_column, num_domains, linear_in_forward=False)
        self.out = _OutBias()
        inputs_dim = _field_count(dnn_feature_columns) * self.embedding.embedding_size + _dense_dim(dnn_feature_columns)
        self.head = StarHead(inputs_dim, dnn_hidden_units, num_domains, use_domain_bn, init_std, dnn_activation, dnn_dropout, dnn_use_bn)
        self._finish()

    def state_dict(self, *args, **kwargs):
        # (star.py's two shared normalisation parameters belong to the model itself, so its state_dict lists them first)
        sd = super().state_dict(*args, **kwargs)
        prefix = kwargs.get("prefix", "")
        out = OrderedDict((prefix + k, sd[prefix + k]) for k in ("shared_bn_weight", "shared_bn_bias"))
        out.update((k, v) for k, v in sd.items() if k not in out)
        if hasattr(sd, "_metadata"):
            out._metadata = sd._metadata
        return out


# ---- the ten further siblings: the same recipe over the remaining heads ----------------------------------------------------------
_TRANS_WORDS = ("usemetatrans", "metatrans", "usetrans")      # MetaNet / attention in front of the head: not built here


def _refuse_options(what, **pairs):
    """`name=(value, the only value served)`: NotImplementedError naming the first option that differs."""
    for name, (val, served) in pairs.items():
        if val != served:
            raise NotImplementedError(f"{what}: {name}={val!r} is not built")


def _check_tasks(what, flag, task_types, task_names, domain_column):
    """MMOE's checks, for the models behind mtl_basemodel.py with one task per scenario."""
    _refuse_flag(flag, _TRANS_WORDS)
    if len(task_types) != len(task_names):
        raise ValueError("num_tasks must be equal to the length of task_types")
    for task_type in task_types:
        if task_type not in ('binary', 'regression'):
            raise ValueError("task must be binary or regression, {} is illegal".format(task_type))
    if len(set(task_types)) > 1:
        raise NotImplementedError(f"task_types {list(task_types)}: every task takes the same type")
    if domain_column is None:
        raise ValueError(f"{what}: domain_column names the column whose id picks a row's task")


class xDeepFM(HeadModel):
    """models/xdeepfm.py: logit = linear_model(X) + cin_linear(cin(emb)) + dnn_linear(dnn(dnn_input))."""

    def __init__(self, linear_feature_columns, dnn_feature_columns, dnn_hidden_units=(256, 256), cin_layer_size=(256, 128,),
                 cin_split_half=True, cin_activation='relu', l2_reg_linear=0.00001, l2_reg_embedding=0.00001, l2_reg_dnn=0,
                 l2_reg_cin=0, init_std=0.0001, seed=1024, dnn_dropout=0, dnn_activation='relu', dnn_use_bn=False, task='binary',
                 device='cpu', gpus=None, flag=None, domain_column=None, num_domains=None, meta_dnn_hidden_units=(32, 64, 32)):
        _refuse_flag(flag, _TRANS_WORDS)
        _refuse_options("XDeepFMHead", cin_activation=(cin_activation, 'relu'), l2_reg_dnn=(l2_reg_dnn, 0), l2_reg_cin=(l2_reg_cin, 0),
                        dnn_dropout=(dnn_dropout, 0), dnn_activation=(dnn_activation, 'relu'), dnn_use_bn=(dnn_use_bn, False))
        super().__init__(linear_feature_columns, dnn_feature_columns, l2_reg_linear, l2_reg_embedding, init_std, seed, task, device,
                         gpus, flag, domain_column, num_domains)
        self.head = XDeepFMHead(_field_count(dnn_feature_columns), self.embedding.embedding_size, _dense_dim(dnn_feature_columns),
                                dnn_hidden_units, cin_layer_size, cin_split_half, init_std)
        self._finish()

    def _logit(self, X):
        emb, dense = self._inputs(X)
        return self.head(emb, dense, self.linear_model(X))


class NFM(HeadModel):
    """models/nfm.py: logit = linear_model(X) + dnn_linear(dnn(cat(BiInteractionPooling(emb), dense)))."""

    def __init__(self, linear_feature_columns, dnn_feature_columns, dnn_hidden_units=(128, 128), l2_reg_embedding=1e-5,
                 l2_reg_linear=1e-5, l2_reg_dnn=0, init_std=0.0001, seed=1024, bi_dropout=0, dnn_dropout=0, dnn_activation='relu',
                 task='binary', device='cpu', gpus=None, flag=None, domain_column=None, num_domains=None,
                 meta_dnn_hidden_units=(32, 64, 32)):
        _refuse_flag(flag, _TRANS_WORDS)
        super().__init__(linear_feature_columns, dnn_feature_columns, l2_reg_linear, l2_reg_embedding, init_std, seed, task, device,
                         gpus, flag, domain_column, num_domains)
        # (NFMHead itself refuses bi_dropout, dnn_dropout and an activation other than relu)
        self.head = NFMHead(self.embedding.embedding_size, _dense_dim(dnn_feature_columns), dnn_hidden_units, l2_reg_dnn, init_std,
                            bi_dropout, dnn_dropout, dnn_activation)
        self._finish()

    def _logit(self, X):
        emb, dense = self._inputs(X)
        return self.head(emb, dense, self.linear_model(X))


class AFM(HeadModel):
    """models/afm.py: logit = linear_model(X) + AFMLayer(emb); with use_attention=False the FM term in its place (DeepFMHead
    without a DNN).  Dense columns reach the linear term only, as in the reference."""

    def __init__(self, linear_feature_columns, dnn_feature_columns, use_attention=True, attention_factor=8, l2_reg_linear=1e-5,
                 l2_reg_embedding=1e-5, l2_reg_att=1e-5, afm_dropout=0, init_std=0.0001, seed=1024, task='binary', device='cpu',
                 gpus=None, flag=None, domain_column=None, num_domains=None, meta_dnn_hidden_units=(32, 64, 32)):
        _refuse_flag(flag, _TRANS_WORDS)
        super().__init__(linear_feature_columns, dnn_feature_columns, l2_reg_linear, l2_reg_embedding, init_std, seed, task, device,
                         gpus, flag, domain_column, num_domains)
        self.use_attention = bool(use_attention)
        if self.use_attention:
            self.head = AFMHead(self.embedding.embedding_size, attention_factor, l2_reg_att, afm_dropout)
        else:
            self.head = DeepFMHead(_field_count(dnn_feature_columns), self.embedding.embedding_size, 0, True, (), 0, init_std)
        self._finish()

    def _logit(self, X):
        emb, _ = self._inputs(X)
        if self.use_attention:
            return self.head(emb, self.linear_model(X))
        return self.head(emb, None, self.linear_model(X))


class AutoInt(HeadModel):
    """models/autoint.py: logit = dnn_linear(cat(int_layers(emb), dnn(dnn_input))).  As in the reference (autoint.py:46, :89-90)
    `linear_model` exists with l2 0 and stays out of the logit."""

    def __init__(self, linear_feature_columns, dnn_feature_columns, att_layer_num=3, att_head_num=2, att_res=True,
                 dnn_hidden_units=(256, 128), dnn_activation='relu', l2_reg_dnn=0, l2_reg_embedding=1e-5, dnn_use_bn=False,
                 dnn_dropout=0, init_std=0.0001, seed=1024, task='binary', device='cpu', gpus=None, flag=None, domain_column=None,
                 num_domains=None, meta_dnn_hidden_units=(32, 64, 32)):
        _refuse_flag(flag, _TRANS_WORDS)
        _refuse_options("AutoIntHead", l2_reg_dnn=(l2_reg_dnn, 0))
        super().__init__(linear_feature_columns, dnn_feature_columns, 0, l2_reg_embedding, init_std, seed, task, device, gpus, flag,
                         domain_column, num_domains, linear_in_forward=False)
        self.head = AutoIntHead(_field_count(dnn_feature_columns), self.embedding.embedding_size, _dense_dim(dnn_feature_columns),
                                att_layer_num, att_head_num, att_res, dnn_hidden_units, init_std, dnn_dropout, dnn_activation, dnn_use_bn)
        self._finish()

    def _logit(self, X):
        emb, dense = self._inputs(X)
        return self.head(emb, dense)


class FiBiNET(HeadModel):
    """models/fibinet.py: logit = linear_model(X) + dnn_linear(dnn(cat(Bilinear(SE(emb)), Bilinear(emb), dense))).  The
    reference registers no regulariser of its own (`l2_reg_dnn` reaches nothing there, and nothing here)."""

    def __init__(self, linear_feature_columns, dnn_feature_columns, bilinear_type='interaction', reduction_ratio=3,
                 dnn_hidden_units=(128, 128), l2_reg_linear=1e-5, l2_reg_embedding=1e-5, l2_reg_dnn=0, init_std=0.0001, seed=1024,
                 dnn_dropout=0, dnn_activation='relu', task='binary', device='cpu', gpus=None, flag=None, domain_column=None,
                 num_domains=None, meta_dnn_hidden_units=(32, 64, 32)):
        _refuse_flag(flag, _TRANS_WORDS)
        super().__init__(linear_feature_columns, dnn_feature_columns, l2_reg_linear, l2_reg_embedding, init_std, seed, task, device,
                         gpus, flag, domain_column, num_domains)
        self.head = FiBiNETHead(_field_count(dnn_feature_columns), self.embedding.embedding_size, _dense_dim(dnn_feature_columns),
                                bilinear_type, reduction_ratio, dnn_hidden_units, l2_reg_linear, init_std, dnn_dropout, dnn_activation)
        self._finish()

    def _logit(self, X):
        emb, dense = self._inputs(X)
        # (fibinet.py:118-121: without linear columns the logit is the DNN's alone)
        return self.head(emb, dense, self.linear_model(X) if self.linear_feature_columns else None)


class PNN(HeadModel):
    """models/pnn.py: logit = dnn_linear(dnn(cat(flatten(emb), inner products, outer products, dense))).  No linear columns."""

    def __init__(self, dnn_feature_columns, dnn_hidden_units=(128, 128), l2_reg_embedding=1e-5, l2_reg_dnn=0, init_std=0.0001,
                 seed=1024, dnn_dropout=0, dnn_activation='relu', use_inner=True, use_outter=False, kernel_type='mat', task='binary',
                 device='cpu', gpus=None, flag=None, domain_column=None, num_domains=None, meta_dnn_hidden_units=(32, 64, 32)):
        _refuse_flag(flag, _TRANS_WORDS)
        if kernel_type not in ('mat', 'vec', 'num'):
            raise ValueError("kernel_type must be mat,vec or num")
        super().__init__([], dnn_feature_columns, 0, l2_reg_embedding, init_std, seed, task, device, gpus, flag, domain_column,
                         num_domains, linear_in_forward=False)
        self.head = PNNHead(_field_count(dnn_feature_columns), self.embedding.embedding_size, _dense_dim(dnn_feature_columns),
                            dnn_hidden_units, use_inner, use_outter, kernel_type, l2_reg_dnn, init_std, dnn_dropout, dnn_activation)
        self._finish()

    def _logit(self, X):
        emb, dense = self._inputs(X)
        return self.head(emb, dense)


class AdaSparse(HeadModel):
    """models/adasparse.py: logit = dnn_linear(pruned_dnn(dnn_input, domain_emb)), where domain_emb is the scenario column's own
    field of the looked-up embeddings (adasparse.py:166-167): a slice of `emb`, so autograd adds both gradient paths back into
    the table.  `linear_model` exists, is regularised and stays out of the logit.  The reference builds its base class without
    `domain_column` (:135-137), so it has no meta modules; nothing here has either."""

    def __init__(self, linear_feature_columns, dnn_feature_columns, dnn_hidden_units=(256, 128), l2_reg_linear=1e-5,
                 l2_reg_embedding=1e-5, l2_reg_dnn=0, init_std=0.0001, seed=1024, dnn_dropout=0, dnn_activation='relu',
                 dnn_use_bn=False, task='binary', device='cpu', gpus=None, flag=None, domain_column=None, num_domains=None,
                 domain_emb_dim=32):
        _refuse_flag(flag, _TRANS_WORDS)
        _refuse_options("AdaSparseHead", l2_reg_dnn=(l2_reg_dnn, 0))
        if domain_column is None:
            raise ValueError("AdaSparse: domain_column names the column whose embedding steers the pruners")
        super().__init__(linear_feature_columns, dnn_feature_columns, l2_reg_linear, l2_reg_embedding, init_std, seed, task, device,
                         gpus, flag, domain_column, num_domains, linear_in_forward=False)
        from .inputs import split_columns
        sparse = [c.name for c in split_columns(self.dnn_feature_columns)[0]]
        if domain_column not in sparse:
            raise ValueError(f"AdaSparse: domain_column {domain_column!r} is no sparse column of dnn_feature_columns")
        if domain_emb_dim != self.embedding.embedding_size:
            raise ValueError(f"AdaSparse: domain_emb_dim {domain_emb_dim} must equal the embedding width "
                             f"{self.embedding.embedding_size}: domain_emb is the scenario column's own embedding")
        self._domain_field = sparse.index(domain_column)
        inputs_dim = _field_count(dnn_feature_columns) * self.embedding.embedding_size + _dense_dim(dnn_feature_columns)
        self.head = AdaSparseHead(inputs_dim, dnn_hidden_units, domain_emb_dim, init_std, dnn_activation, dnn_dropout, dnn_use_bn)
        self._finish()

    def _logit(self, X):
        emb, dense = self._inputs(X)
        flat = emb.flatten(1)
        return self.head(flat if dense is None else torch.cat([flat, dense], dim=1), emb[:, self._domain_field, :])


class SharedBottom(_ScenarioModel):
    """models/sharedbottom.py behind models/mtl_basemodel.py, one task per scenario, as MMOE: SharedBottomHead returns each row's
    own task logit.  predict -> [n]."""
    returns_column = False

    def __init__(self, dnn_feature_columns, bottom_dnn_hidden_units=(256, 128), tower_dnn_hidden_units=(64,), l2_reg_linear=0.00001,
                 l2_reg_embedding=0.00001, l2_reg_dnn=0, init_std=0.0001, seed=1024, dnn_dropout=0, dnn_activation='relu',
                 dnn_use_bn=False, task_types=('binary', 'binary'), task_names=('ctr', 'ctcvr'), device='cpu', gpus=None,
                 domain_column=None, flag=None):
        _check_tasks("SharedBottom", flag, task_types, task_names, domain_column)
        _refuse_options("SharedBottomHead", l2_reg_dnn=(l2_reg_dnn, 0))
        super().__init__([], dnn_feature_columns, l2_reg_linear, l2_reg_embedding, init_std, seed, task_types[0] if task_types else 'binary',
                         device, gpus, flag, domain_column, len(task_names), linear_in_forward=False)
        self.num_tasks, self.task_names = len(task_names), tuple(task_names)
        inputs_dim = _field_count(dnn_feature_columns) * self.embedding.embedding_size + _dense_dim(dnn_feature_columns)
        self.head = SharedBottomHead(inputs_dim, self.num_tasks, bottom_dnn_hidden_units, tower_dnn_hidden_units, init_std,
                                     dnn_activation, dnn_dropout, dnn_use_bn)
        self._finish()


class PLE(_ScenarioModel):
    """models/ple.py behind models/mtl_basemodel.py, one task per scenario, as MMOE: PLEHead returns each row's own task logit.
    predict -> [n]."""
    returns_column = False

    def __init__(self, dnn_feature_columns, shared_expert_num=1, specific_expert_num=1, num_levels=2, expert_dnn_hidden_units=(256, 128),
                 gate_dnn_hidden_units=(64,), tower_dnn_hidden_units=(64,), l2_reg_linear=0.00001, l2_reg_embedding=0.00001,
                 l2_reg_dnn=0, init_std=0.0001, seed=1024, dnn_dropout=0, dnn_activation='relu', dnn_use_bn=False,
                 task_types=('binary', 'binary'), task_names=('ctr', 'ctcvr'), device='cpu', gpus=None, domain_column=None, flag=None):
        _check_tasks("PLE", flag, task_types, task_names, domain_column)
        _refuse_options("PLEHead", l2_reg_dnn=(l2_reg_dnn, 0))
        super().__init__([], dnn_feature_columns, l2_reg_linear, l2_reg_embedding, init_std, seed, task_types[0] if task_types else 'binary',
                         device, gpus, flag, domain_column, len(task_names), linear_in_forward=False)
        self.num_tasks, self.task_names = len(task_names), tuple(task_names)
        inputs_dim = _field_count(dnn_feature_columns) * self.embedding.embedding_size + _dense_dim(dnn_feature_columns)
        self.head = PLEHead(inputs_dim, self.num_tasks, shared_expert_num, specific_expert_num, num_levels, expert_dnn_hidden_units,
                            gate_dnn_hidden_units, tower_dnn_hidden_units, init_std, dnn_activation, dnn_dropout, dnn_use_bn)
        self._finish()


class ESMM(HeadModel):
    """models/esmm.py behind models/mtl_basemodel.py: ESMMHead returns the probabilities (p_ctr, p_ctr * p_cvr) of every row, and
    a row's loss and prediction are taken on the column of its own task - the masked per-task loss sum (mtl_basemodel.py:268-269)
    and predict's assembly (:376-378) - by RoutedPointLoss with the linear prediction kind, in one launch.  A row whose id is
    neither of the two tasks' takes part in no loss and predicts 0, as in the reference.  Exactly two tasks, binary only, no
    `flag` parameter (esmm.py:38-57).  predict -> [n].  dnn_dropout is ESMMHead's (the kernels' own masks)."""
    returns_column = False
    uses_domains = True

    def __init__(self, dnn_feature_columns, tower_dnn_hidden_units=(256, 128), l2_reg_linear=0.00001, l2_reg_embedding=0.00001,
                 l2_reg_dnn=0, init_std=0.0001, seed=1024, dnn_dropout=0, dnn_activation='relu', dnn_use_bn=False,
                 task_types=('binary', 'binary'), task_names=('ctr', 'ctcvr'), device='cpu', gpus=None, domain_column=None):
        if len(task_names) != 2:
            raise ValueError("the length of task_names must be equal to 2")
        if len(dnn_feature_columns) == 0:
            raise ValueError("dnn_feature_columns is null!")
        if len(task_types) != 2:
            raise ValueError("num_tasks must be equal to the length of task_types")
        for task_type in task_types:
            if task_type != 'binary':
                raise ValueError("task must be binary in ESMM, {} is illegal".format(task_type))
        if domain_column is None:
            raise ValueError("ESMM: domain_column names the column whose id picks a row's task")
        super().__init__([], dnn_feature_columns, l2_reg_linear, l2_reg_embedding, init_std, seed, 'binary', device, gpus, None,
                         domain_column, 2, linear_in_forward=False)
        self.num_tasks, self.task_names = 2, tuple(task_names)
        inputs_dim = _field_count(dnn_feature_columns) * self.embedding.embedding_size + _dense_dim(dnn_feature_columns)
        self.head = ESMMHead(inputs_dim, tower_dnn_hidden_units, l2_reg_dnn, init_std, dnn_dropout, dnn_activation, dnn_use_bn)
        self._routed = RoutedPointLoss("binary_crossentropy", "regression")
        self._finish()

    def compile(self, optimizer, loss=None, metrics=None):
        super().compile(optimizer, loss, metrics)
        self._routed = RoutedPointLoss(self.loss_func, "regression")      # (the head's outputs are probabilities already)

    def _task_ids(self, X):
        return self._domain_ids(X).long() - self.domain_id_offset

    def _loss_and_pred(self, X, y=None):
        return self._routed(self.head(self._dnn_input(X)), self._task_ids(X), y)
