"""Fit a signed distance field to a triangle mesh and write its zero level set
back as a mesh (the reference's main_sdf.py).

    python main_sdf.py armadillo.obj --workspace trial_sdf
    python main_sdf.py armadillo.obj --workspace trial_sdf --test

The mesh (.obj or .ply) is prepared once on the host; every step's 2^18
points are drawn from it and signed on the device (sdf/provider.py,
csrc/sdf.hip). Training ends with <workspace>/results/output.ply; --test loads
<workspace>/checkpoints/ngp.pth and writes only the mesh. DESIGN.md §21.
"""
import argparse
import os


def main(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument("path", type=str)
    parser.add_argument("--test", action="store_true", help="test mode")
    parser.add_argument("--workspace", type=str, default="workspace")
    parser.add_argument("--seed", type=int, default=0)
    parser.add_argument("--lr", type=float, default=1e-4, help="initial learning rate")
    parser.add_argument("--fp16", action="store_true", help="accepted; mixed precision is always on")
    parser.add_argument("--ff", action="store_true", help="accepted; the fully-fused MLP is always on")
    parser.add_argument("--tcnn", action="store_true", help="rejected: there is no TCNN backend here")
    parser.add_argument("--num_samples", type=int, default=2 ** 18, help="points per step")
    parser.add_argument("--epochs", type=int, default=20)
    parser.add_argument("--steps_per_epoch", type=int, default=100)
    parser.add_argument("--mesh_resolution", type=int, default=512,
                        help="lattice of the exported mesh (the reference's 1024 is a 4 GB volume here)")
    opt = parser.parse_args(argv)
    if opt.tcnn:
        parser.error("--tcnn: there is no TCNN backend; the fully-fused MLP (--ff) is the only one")
    print(opt)

    import torch

    from sdf import SDFDataset, SDFNetwork, SDFTrainer, prepare_mesh, read_mesh, seed_everything

    seed_everything(opt.seed)
    device = torch.device("cuda")
    model = SDFNetwork(encoding="hashgrid").to(device)
    print(model)
    out = os.path.join(opt.workspace, "results", "output.ply")

    if opt.test:
        trainer = SDFTrainer(model, None, workspace=opt.workspace, lr=opt.lr)
        trainer.load_checkpoint(model_only=True)
        trainer.save_mesh(out, opt.mesh_resolution)
        return trainer

    vertices, faces = read_mesh(opt.path)
    mesh = prepare_mesh(vertices, faces, device=device)
    print(f"[INFO] mesh: {mesh.vertices.shape} {mesh.faces.shape}")
    dataset = SDFDataset(mesh, num_samples=opt.num_samples, seed=opt.seed)
    trainer = SDFTrainer(model, dataset, workspace=opt.workspace, lr=opt.lr, epochs=opt.epochs,
                         steps_per_epoch=opt.steps_per_epoch)
    trainer.train()
    trainer.save_checkpoint()
    trainer.save_mesh(out, opt.mesh_resolution)  # also test
    return trainer


if __name__ == "__main__":
    main()
