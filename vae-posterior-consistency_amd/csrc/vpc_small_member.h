// (tile, member) of an ensemble workgroup and member g's arguments built in registers: the HEAD of the ensemble kernels of
// vpc_small.hip, included as text into step_small_multi_kernel, step_small_multi_aug_kernel and step_small_multi_eddi_kernel in
// front of the tile body (vpc_small_body.h), for the reason given there - one piece of code, and a kernel that compiles to the
// instructions it had with these lines spelled out in it.
// In scope at the point of inclusion: `ma` (the kernel argument: a SmallMultiArgs, or a record derived from it) and the flags AUG
// and PN and `MemberHow` (MemberEarly / MemberLate of vpc_small.hip).  Leaves `a` (a MemberArgs: the fields of SmallArgs as the tile body names them), `mem` and `const unsigned tile_id`.
// (No include guard: a code fragment, included once per kernel.)
    // (tile, member) of this workgroup.  Workgroups are dealt round-robin over the 8 XCDs by their linear id (x fastest).
    //   order 0: grid (tiles, G), id = g * tiles + t - the tiles of a member land on different XCDs, every L2 sees every
    //            member's images;
    //   order 1: grid (8 x tiles, ceil(G / 8)), t = x / 8, g = 8 y + x % 8 - all tiles of a member sit on ids of one residue
    //            mod 8, so a member's images are read through ONE L2 (the surplus workgroups of the last member group return).
    unsigned mem, tile_;
    if (ma.order == 0) {
        mem = blockIdx.y;
        tile_ = blockIdx.x;
    } else {
        tile_ = blockIdx.x >> 3;
        mem = 8 * blockIdx.y + (blockIdx.x & 7);
        if (mem >= ma.G) return;
    }
    const VpcMember* r = ma.members + mem;  // (uniform address: scalar loads)
    const SmallArgs& b = ma.base;
    MemberArgsOf<MemberHow> a;
    a.x = b.x + mem * ma.sx;
    a.enc_img = b.enc_img + mem * ma.simg;
    a.dec_img = b.dec_img + mem * ma.simg;
    a.m.v0 = b.m[0] + mem * ma.sm;
    a.m.v1 = b.m[1] ? b.m[1] + mem * ma.smp : nullptr;
    MemberHow::second_mask(a, mem, r);  // mB
    a.cA.v0 = r->co.cA[0]; a.cA.v1 = r->co.cA[1]; a.cE.v0 = r->co.cE[0]; a.cE.v1 = r->co.cE[1];
    MemberHow::planes_and_blocks(a, ma, mem);  // eps, eps_ml, partE, partD, loss_part
    a.bq = r->co.bq; a.bp = r->co.bp; a.cr = r->co.cr; a.wml = r->co.wml; a.inv_B = b.inv_B; a.x_logvar = b.x_logvar;
    a.B = b.B; a.d = b.d; a.L = b.L; a.npass = b.npass;
    a.draw = b.draw;
    a.d_real = (AUG || PN) ? b.d_real : b.d;  // (obs_dim under the row pitch d: read by the mask-augmented and point-net stages only)
    // (the draws are those of an unsharded stand-alone step - no device-side state, element offset 0, all B rows local: derived
    // from eps[0], mask, B and constants instead of carried in registers)
    a.mask_in = b.mask_in ? a.m.v0 : nullptr;
    a.keep_prob = r->keep_prob;
    a.eps_out = const_cast<float*>(MemberHow::plane0(a, ma, mem));
    a.n_eps = b.n_eps;
    a.seed = r->seed; a.off_mask = b.off_mask; a.off_eps = b.off_eps;
    a.state = nullptr; a.mask_elem_lo = 0; a.shard = EpsShard{b.B, b.B, 0, 16};
    const unsigned tile_id = tile_;
