"""utils/visualization.py: the embedding plots of a trained model.  `Visualization(model, config, vis_opts)` samples
`config.disp_triple_num` validation triples, takes the rows `model.embed(h, r, t)` returns for each, reduces them to 2-D and draws
up to three pictures -- entities, relations, and entities with relations -- as the reference does.  The reduction is
Evaluator.project_vectors (exact t-SNE on the device, csrc/kge_tsne.hip) instead of sklearn.manifold.TSNE; drawing needs matplotlib
only.  `plot_train_result` / `plot_test_result` (loss curves, LaTeX tables over the result files) are not built."""
import os

import numpy as np
import torch

from .evaluator import Evaluator, _as_array
from .state import _log


class Visualization:
    def __init__(self, model, config, vis_opts=None, evaluator=None, seed=None):
        opts = vis_opts or {}
        self.ent_only_plot = bool(opts.get("ent_only_plot", False))
        self.rel_only_plot = bool(opts.get("rel_only_plot", False))
        self.ent_and_rel_plot = bool(opts.get("ent_and_rel_plot", False))
        self.model = model
        self.config = config
        self.evaluator = evaluator
        self.seed = int(getattr(config, "seed", 0) or 0) if seed is None else int(seed)
        self.h_name, self.r_name, self.t_name = [], [], []
        self.h_emb, self.r_emb, self.t_emb = [], [], []
        self.h_proj_emb, self.r_proj_emb, self.t_proj_emb = [], [], []
        if self.model is not None:
            kg = self.config.knowledge_graph
            self.validation_triples_ids = kg.read_cache_data('triplets_valid')
            self.idx2entity = kg.read_cache_data('idx2entity')
            self.idx2relation = kg.read_cache_data('idx2relation')
            if self.evaluator is None:
                self.evaluator = Evaluator(model, config)
            self.get_idx_n_emb()

    def _rows(self, h, r, t):
        """The (head, relation, tail) rows of one triple, [1, D] each: model.embed's where it returns exactly these three (the
        reference's contract), else the rows of the matrices the neighbour search compares (models of several tables)."""
        dev = self.config.device
        ids = [torch.as_tensor([int(x)], dtype=torch.int64, device=dev) for x in (h, r, t)]
        with torch.no_grad():
            out = self.model.embed(*ids)
            if isinstance(out, (tuple, list)) and len(out) == 3 and all(isinstance(x, torch.Tensor) and x.dim() == 2 for x in out):
                return tuple(x.detach().float() for x in out)
            ent, rel = self.model.entity_matrix(), self.model.relation_matrix()
            return ent[ids[0]], rel[ids[1]], ent[ids[2]]

    def get_idx_n_emb(self):
        """visualization.py:78-104: the sampled triples' names and rows (drawn with replacement, from config.seed)."""
        n = int(self.config.disp_triple_num)
        valid = _as_array(self.validation_triples_ids, len(self.validation_triples_ids))
        rng = np.random.default_rng(self.seed)
        for h, r, t in valid[rng.choice(len(valid), n)]:
            self.h_name.append(self.idx2entity[int(h)])
            self.r_name.append(self.idx2relation[int(r)])
            self.t_name.append(self.idx2entity[int(t)])
            eh, er, et = self._rows(h, r, t)
            self.h_emb.append(eh)
            self.r_emb.append(er)
            self.t_emb.append(et)
            if self.ent_and_rel_plot:
                self.h_proj_emb.append(eh)
                self.r_proj_emb.append(er)
                self.t_proj_emb.append(et)

    @staticmethod
    def perplexity_for(n):
        """sklearn's default of 30, clamped so that 3 x perplexity neighbours exist among n points (sklearn refuses 30 for the
        reference's default of 20 points)."""
        return float(min(30.0, max(1.0, (n - 1) / 3.0)))

    def _reduce(self, x, **kw):
        n = int(x.shape[0])
        kw.setdefault("perplexity", self.perplexity_for(n))
        _log("\t Reducing dimension using TSNE to 2! (%d points, perplexity %g)" % (n, kw["perplexity"]))
        return self.evaluator.project_vectors(x, **kw).cpu().numpy()

    def plot_embedding(self, resultpath=None, algos=None, show_label=False, disp_num_r_n_e=20, project_only=False, **tsne):
        """visualization.py:106-154.  One PNG per enabled plot under `resultpath`: <algos>_entity_plot, <algos>_rel_plot,
        <algos>_ent_n_rel_plot.  project_only: nothing is drawn; -> {plot stem: (coords numpy [n, 2], names)} either way.  Further
        keywords go to Evaluator.project_vectors."""
        assert self.model is not None, 'Please provide a model!'
        algos = str(algos if algos is not None else getattr(self.model, "model_name", "model"))
        out = {}
        if self.ent_only_plot:
            x = self._reduce(torch.cat(self.h_emb + self.t_emb, dim=0), **tsne)
            names = np.asarray(list(self.h_name) + list(self.t_name))
            out[algos + '_entity_plot'] = (x, names)
            if not project_only:
                self.draw_embedding(x, names, resultpath, algos + '_entity_plot', show_label)
        if self.rel_only_plot:
            x = self._reduce(torch.cat(self.r_emb, dim=0), **tsne)
            names = np.asarray(self.r_name)
            out[algos + '_rel_plot'] = (x, names)
            if not project_only:
                self.draw_embedding(x, names, resultpath, algos + '_rel_plot', show_label)
        if self.ent_and_rel_plot:
            m = len(self.h_proj_emb)
            rows = self.h_proj_emb + self.r_proj_emb + self.t_proj_emb
            if len({int(r.shape[1]) for r in rows}) != 1:
                _log("plot_embedding: entity and relation rows differ in width (%s); no %s_ent_n_rel_plot"
                     % (sorted({int(r.shape[1]) for r in rows}), algos))
            else:
                x = self._reduce(torch.cat(rows, dim=0), **tsne)
                d = int(disp_num_r_n_e)
                parts = (x[:m][:d], x[m:2 * m][:d], x[2 * m:3 * m][:d])
                names = (self.h_name[:d], self.r_name[:d], self.t_name[:d])
                out[algos + '_ent_n_rel_plot'] = (np.concatenate(parts), np.asarray(sum((list(s) for s in names), [])))
                if not project_only:
                    self.draw_embedding_rel_space(*parts, *names, resultpath, algos + '_ent_n_rel_plot', show_label)
        return out

    @staticmethod
    def _pyplot():
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
        return plt

    @staticmethod
    def _save(plt, fig, resultpath, name):
        os.makedirs(str(resultpath), exist_ok=True)
        path = os.path.join(str(resultpath), name + '.png')
        fig.savefig(path, bbox_inches='tight', dpi=150)
        plt.close(fig)
        return path

    def draw_embedding(self, embs, names, resultpath, algos, show_label):
        """visualization.py:333-367: one scatter, a colour per point, the names beside the points when show_label."""
        plt = self._pyplot()
        fig, ax = plt.subplots()
        colours = plt.cm.tab20(np.arange(len(embs)) % 20)
        ax.scatter(embs[:, 0], embs[:, 1], c=colours, s=30)
        if show_label:
            for (x, y), name in zip(embs, names):
                ax.annotate(str(name), (x, y), fontsize=6)
        ax.set_title(algos)
        return self._save(plt, fig, resultpath, algos)

    def draw_embedding_rel_space(self, h_emb, r_emb, t_emb, h_name, r_name, t_name, resultpath, algos, show_label):
        """visualization.py:369-427: heads, relations and tails in one picture, an arrow head -> relation -> tail per triple."""
        plt = self._pyplot()
        fig, ax = plt.subplots()
        for emb, colour, marker, label in ((h_emb, "tab:red", "o", "head"), (r_emb, "tab:green", "^", "relation"),
                                           (t_emb, "tab:blue", "s", "tail")):
            ax.scatter(emb[:, 0], emb[:, 1], c=colour, marker=marker, s=30, label=label)
        for i in range(len(h_emb)):
            ax.plot([h_emb[i, 0], r_emb[i, 0], t_emb[i, 0]], [h_emb[i, 1], r_emb[i, 1], t_emb[i, 1]], c="0.6", lw=0.5)
            if show_label:
                for (x, y), name in ((h_emb[i], h_name[i]), (r_emb[i], r_name[i]), (t_emb[i], t_name[i])):
                    ax.annotate(str(name), (x, y), fontsize=6)
        ax.legend(fontsize=7)
        ax.set_title(algos)
        return self._save(plt, fig, resultpath, algos)
