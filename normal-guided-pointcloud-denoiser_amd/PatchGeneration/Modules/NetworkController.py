"""Checkpoints and the training loop (drop-in for Network and NetworkTrainer of PatchGeneration/Modules/
NetworkController.py).

`Network(model)` holds a Network.GCNModel.DGCNN or BetterDGCNN and saves / loads its state dict under the reference's `.t7` rules
(NetworkController.py:28-52).  `NetworkTrainer(network, batches).train(epochs, ...)` is the training half of
NetworkTrainer.train (NetworkController.py:94-139): per batch `train()`, forward, the cosine and MSE losses weighted
by `loss_based_on_value_loss`, `backward()`, one Adam step -- on a model built with `trainable=True`, whose
convolutions run forward and backward on the HIP kernels of csrc/dgcnn_train.hip.

Not here: the reference's DatasetManager / data loaders (`batches` is any iterable of device or host batches, for
instance PatchDataset.trainingBatches), its tensorboard summaries, its validation pass and per-epoch checkpoints
(call `Network.saveModel` when one is wanted), and NetworkUser (PatchCollector.predictNormals does that job).
"""
from __future__ import annotations

import os
from pathlib import Path

import torch
import torch.nn.functional as F

import pcd_native as _nat

from .Network.GCNModel import DGCNN, BetterDGCNN


class Network:
    def __init__(self, model):
        if not isinstance(model, DGCNN) and not isinstance(model, BetterDGCNN):
            raise ValueError("A Network is instantiated with a model that is not a member of DGCNN.\n"
                             f"Current type: {type(model)}")
        self.model = model

    def getModel(self):
        return self.model

    def setModel(self, model):
        self.model = model

    def saveModel(self, target_path):
        """The model's state dict to a new `.t7` file (parent directories are made; an existing file is refused)."""
        if not type(target_path) == str:
            raise ValueError("target_path is not a string..")
        if not target_path.endswith(".t7"):
            raise ValueError("target_path should end with .t7 to save the current weights with the correct file extension.")
        if os.path.isfile(target_path):
            raise ValueError("Attempting to write over an existing save file.")
        Path(target_path).parent.mkdir(parents=True, exist_ok=True)
        torch.save(self.model.state_dict(), target_path)

    def loadModel(self, target_path):
        """A `.t7` state dict into the model (strict: a missing or unexpected key raises)."""
        if not type(target_path) == str:
            raise ValueError("target_path should be a string.")
        if not os.path.isfile(target_path):
            raise ValueError("target_path should be a path to a file.")
        if not target_path.endswith(".t7"):
            raise ValueError("target_path should be a path to a .t7 file.")
        device = next(self.model.parameters()).device
        self.model.load_state_dict(torch.load(target_path, map_location=device, weights_only=True))


class NetworkTrainer:
    def __init__(self, network, batches):
        """batches: an iterable (gone through once per epoch) of (inputs [b, 64, 20], gt [b, 3]) tensors -- the rows
        as collectNetworkInput gives them and the ground-truth normals in the patches' aligned frame."""
        if not isinstance(network, Network):
            raise ValueError("A NetworkTrainer is instantiated with a network that is not a member of Network.\n"
                             f"Current type: {type(network)}")
        if not hasattr(batches, "__iter__") or isinstance(batches, torch.Tensor):
            raise ValueError(f"batches should be an iterable of (inputs, gt) pairs. Current type: {type(batches)}")
        self.network = network
        self.data = batches

    def train(self, epochs, Adam_learning_rate=0.0001, Adam_betas=(0.9, 0.999), loss_based_on_value_loss=1.):
        """Trains the network's model in place and returns the per-step losses: a list of (cos_loss, value_loss)
        floats, read from the device once, after the last step."""
        if type(epochs) != int or epochs < 1:
            raise ValueError("epochs should be an integers higher than zero being the amount of epochs you want to "
                             f"train. Currently it is {epochs}")
        if type(Adam_learning_rate) != float or Adam_learning_rate ** 2 > 1:
            raise ValueError(f"Adam_learning_rate should be a number between 0 and 1. Currently it is {Adam_learning_rate}")
        if type(Adam_betas) != tuple or len(Adam_betas) != 2 or any(type(x) != float for x in Adam_betas) \
                or any(x ** 2 > 1 for x in Adam_betas) or Adam_betas[0] > Adam_betas[1]:
            raise ValueError("Adam_betas should be a tuple of 2 floats between 0 and 1 with the first value lower than "
                             f"the second value. Currently it is {Adam_betas}")
        if not isinstance(loss_based_on_value_loss, (float, int)) or not 0 <= loss_based_on_value_loss <= 1:
            raise ValueError("loss_based_on_value_loss should be a number between 0 and 1. Currently it is "
                             f"{loss_based_on_value_loss}")
        dgcnn = self.network.getModel()
        if not dgcnn.trainable:
            raise ValueError("NetworkTrainer: the model was built without trainable=True")
        dev = _nat.device()
        dgcnn.to(dev)
        optimizer = torch.optim.Adam(dgcnn.parameters(), lr=Adam_learning_rate, betas=Adam_betas)
        weight_alpha = 1 - loss_based_on_value_loss
        weight_beta = loss_based_on_value_loss
        losses = []
        for _ in range(epochs):
            for inputs, gt_norm in self.data:
                inputs = torch.as_tensor(inputs).to(dev, torch.float32).permute(0, 2, 1).contiguous()
                gt_norm = torch.as_tensor(gt_norm).to(dev, torch.float32)
                cos_target = torch.ones(inputs.size(0), dtype=torch.float32, device=dev)
                optimizer.zero_grad()
                dgcnn.train()
                output = dgcnn(inputs)
                cos_loss = F.cosine_embedding_loss(output, gt_norm, cos_target)
                value_loss = F.mse_loss(output, gt_norm)
                loss = weight_alpha * cos_loss + weight_beta * value_loss
                loss.backward()
                optimizer.step()
                losses.append(torch.stack((cos_loss.detach(), value_loss.detach())))
        self.network.setModel(dgcnn)
        if not losses:
            return []
        return [(float(c), float(v)) for c, v in torch.stack(losses).cpu().tolist()]
