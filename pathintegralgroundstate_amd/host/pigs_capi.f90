!-----------------------------------------------------------------------
! pigs_capi -- ISO_C_BINDING interface to libpigs_hip.so (include/pigs_hip.h).
!
! This is the Fortran side of the drop-in boundary: a host written in
! Fortran 90 (like the reference) passes its own arrays -- Path(dim,Np,0:2*Nb),
! VTable(0:Nmax+1), LogWF(0:Nmax+1), all real(8), column-major -- unchanged.
! Particle indices are 1-based and bead indices 0-based exactly as in the
! reference; walker indices are 0-based (walkers are new).
! Every function returns 0 on success or a negative pigs_status.
!-----------------------------------------------------------------------
module pigs_capi

  use iso_c_binding
  implicit none

  integer(c_int), parameter :: PIGS_OK = 0

  ! mirrors `struct pigs_params` (the reference's module globals, global_mod.f90:5-12,
  ! system_mod.f90:8-9, plus dt)
  ! mirrors `struct pigs_sweep_params` (device-resident sampler, K6)
  type, bind(C) :: pigs_sweep_params
     integer(c_int32_t) :: Nlev, Nstag, CMFreq, Lstag
     real(c_double)     :: delta_cm
     real(c_double)     :: CWorm, density, rbin
     integer(c_int32_t) :: swapping, Nobdm, Nbin, Npw
     integer(c_int32_t) :: sampling = 0, reserved = 0      ! 0 = 'bis', 1 = 'sta'
  end type pigs_sweep_params

  type, bind(C) :: pigs_params
     integer(c_int32_t) :: dim, Np, Nb, Nmax
     integer(c_int32_t) :: trap, wf_table, v_table, reserved
     real(c_double)     :: dr, rcut2, dt, Rm
     real(c_double)     :: Lbox(3)
     real(c_double)     :: a_ho(3)
  end type pigs_params

  interface

     function pigs_ctx_create(p,VTable,LogWF,n_walkers,device_id,ctx) bind(C,name='pigs_ctx_create') result(rc)
       import :: c_int, c_int32_t, c_double, c_ptr, pigs_params
       type(pigs_params), intent(in) :: p
       real(c_double), intent(in)    :: VTable(*),LogWF(*)
       integer(c_int32_t), value     :: n_walkers,device_id
       type(c_ptr), intent(out)      :: ctx
       integer(c_int) :: rc
     end function pigs_ctx_create

     function pigs_ctx_destroy(ctx) bind(C,name='pigs_ctx_destroy') result(rc)
       import :: c_int, c_ptr
       type(c_ptr), value :: ctx
       integer(c_int) :: rc
     end function pigs_ctx_destroy

     function pigs_last_error() bind(C,name='pigs_last_error') result(msg)
       import :: c_ptr
       type(c_ptr) :: msg
     end function pigs_last_error

     function pigs_device_count(n) bind(C,name='pigs_device_count') result(rc)
       import :: c_int, c_int32_t
       integer(c_int32_t), intent(out) :: n
       integer(c_int) :: rc
     end function pigs_device_count

     function pigs_sync(ctx) bind(C,name='pigs_sync') result(rc)
       import :: c_int, c_ptr
       type(c_ptr), value :: ctx
       integer(c_int) :: rc
     end function pigs_sync

     function pigs_set_tuning(ctx,key,value) bind(C,name='pigs_set_tuning') result(rc)
       import :: c_int, c_int32_t, c_ptr, c_char
       type(c_ptr), value :: ctx
       character(kind=c_char), intent(in) :: key(*)
       integer(c_int32_t), value :: value
       integer(c_int) :: rc
     end function pigs_set_tuning

     function pigs_build_tables(Nmax,Rm,rmax,VTable,LogWF,dr_out) bind(C,name='pigs_build_tables') result(rc)
       import :: c_int, c_int32_t, c_double
       integer(c_int32_t), value :: Nmax
       real(c_double), value     :: Rm,rmax
       real(c_double)            :: VTable(*),LogWF(*),dr_out
       integer(c_int) :: rc
     end function pigs_build_tables

     function pigs_build_tables_kind(kind,Nmax,Rm,rmax,VTable,LogWF,dr_out) &
          & bind(C,name='pigs_build_tables_kind') result(rc)
       import :: c_int, c_int32_t, c_double
       integer(c_int32_t), value :: kind,Nmax
       real(c_double), value     :: Rm,rmax
       real(c_double)            :: VTable(*),LogWF(*),dr_out
       integer(c_int) :: rc
     end function pigs_build_tables_kind

     function pigs_path_upload(ctx,walker,Path) bind(C,name='pigs_path_upload') result(rc)
       import :: c_int, c_int32_t, c_double, c_ptr
       type(c_ptr), value        :: ctx
       integer(c_int32_t), value :: walker
       real(c_double), intent(in) :: Path(*)
       integer(c_int) :: rc
     end function pigs_path_upload

     function pigs_path_download(ctx,walker,Path) bind(C,name='pigs_path_download') result(rc)
       import :: c_int, c_int32_t, c_double, c_ptr
       type(c_ptr), value        :: ctx
       integer(c_int32_t), value :: walker
       real(c_double)            :: Path(*)
       integer(c_int) :: rc
     end function pigs_path_download

     function pigs_path_upload_all(ctx,Paths) bind(C,name='pigs_path_upload_all') result(rc)
       import :: c_int, c_double, c_ptr
       type(c_ptr), value         :: ctx
       real(c_double), intent(in) :: Paths(*)
       integer(c_int) :: rc
     end function pigs_path_upload_all

     function pigs_path_download_all(ctx,Paths) bind(C,name='pigs_path_download_all') result(rc)
       import :: c_int, c_double, c_ptr
       type(c_ptr), value :: ctx
       real(c_double)     :: Paths(*)
       integer(c_int) :: rc
     end function pigs_path_download_all

     ! replaces `call UpdateAction(...)` (reference vpi_mod.f90:2491), batched
     function pigs_delta_action_batch(ctx,n_items,walker,ip,ib,xnew,xold,DeltaS) &
          & bind(C,name='pigs_delta_action_batch') result(rc)
       import :: c_int, c_int32_t, c_int64_t, c_double, c_ptr
       type(c_ptr), value             :: ctx
       integer(c_int64_t), value      :: n_items
       integer(c_int32_t), intent(in) :: walker(*),ip(*),ib(*)
       real(c_double), intent(in)     :: xnew(*),xold(*)
       real(c_double)                 :: DeltaS(*)
       integer(c_int) :: rc
     end function pigs_delta_action_batch

     ! pinned, device-mapped staging arrays owned by the library (low-latency sampler path)
     function pigs_stage_reserve(ctx,capacity,keep,walker,ip,ib,xnew,xold,DeltaS) &
          & bind(C,name='pigs_stage_reserve') result(rc)
       import :: c_int, c_int64_t, c_ptr
       type(c_ptr), value        :: ctx
       integer(c_int64_t), value :: capacity,keep
       type(c_ptr), intent(out)  :: walker,ip,ib,xnew,xold,DeltaS
       integer(c_int) :: rc
     end function pigs_stage_reserve

     function pigs_delta_action_staged(ctx,n_items) bind(C,name='pigs_delta_action_staged') result(rc)
       import :: c_int, c_int64_t, c_ptr
       type(c_ptr), value        :: ctx
       integer(c_int64_t), value :: n_items
       integer(c_int) :: rc
     end function pigs_delta_action_staged

     function pigs_commit_reserve(ctx,capacity,keep,walker,ip,ib,x) bind(C,name='pigs_commit_reserve') result(rc)
       import :: c_int, c_int64_t, c_ptr
       type(c_ptr), value        :: ctx
       integer(c_int64_t), value :: capacity,keep
       type(c_ptr), intent(out)  :: walker,ip,ib,x
       integer(c_int) :: rc
     end function pigs_commit_reserve

     function pigs_commit_staged(ctx,n) bind(C,name='pigs_commit_staged') result(rc)
       import :: c_int, c_int64_t, c_ptr
       type(c_ptr), value        :: ctx
       integer(c_int64_t), value :: n
       integer(c_int) :: rc
     end function pigs_commit_staged

     function pigs_delta_action_parts(ctx,n_items,walker,ip,ib,xnew,xold,parts) &
          & bind(C,name='pigs_delta_action_parts') result(rc)
       import :: c_int, c_int32_t, c_int64_t, c_double, c_ptr
       type(c_ptr), value             :: ctx
       integer(c_int64_t), value      :: n_items
       integer(c_int32_t), intent(in) :: walker(*),ip(*),ib(*)
       real(c_double), intent(in)     :: xnew(*),xold(*)
       real(c_double)                 :: parts(*)
       integer(c_int) :: rc
     end function pigs_delta_action_parts

     ! replaces `Path(k,ip,ib) = xnew(k)` on accept
     function pigs_commit_beads(ctx,n,walker,ip,ib,x) bind(C,name='pigs_commit_beads') result(rc)
       import :: c_int, c_int32_t, c_int64_t, c_double, c_ptr
       type(c_ptr), value             :: ctx
       integer(c_int64_t), value      :: n
       integer(c_int32_t), intent(in) :: walker(*),ip(*),ib(*)
       real(c_double), intent(in)     :: x(*)
       integer(c_int) :: rc
     end function pigs_commit_beads

     function pigs_swap_tails(ctx,walker,iw,ik) bind(C,name='pigs_swap_tails') result(rc)
       import :: c_int, c_int32_t, c_ptr
       type(c_ptr), value        :: ctx
       integer(c_int32_t), value :: walker,iw,ik
       integer(c_int) :: rc
     end function pigs_swap_tails

     ! PotentialEnergy (reference sample_mod.f90:13)
     function pigs_potential_energy_slice(ctx,walker,ib,want_F2,Pot,F2) &
          & bind(C,name='pigs_potential_energy_slice') result(rc)
       import :: c_int, c_int32_t, c_double, c_ptr
       type(c_ptr), value        :: ctx
       integer(c_int32_t), value :: walker,ib,want_F2
       real(c_double)            :: Pot,F2
       integer(c_int) :: rc
     end function pigs_potential_energy_slice

     ! ThermEnergy (reference sample_mod.f90:323)
     function pigs_therm_energy_batch(ctx,n,walkers,E,Ec,Ep) bind(C,name='pigs_therm_energy_batch') result(rc)
       import :: c_int, c_int32_t, c_double, c_ptr
       type(c_ptr), value             :: ctx
       integer(c_int32_t), value      :: n
       integer(c_int32_t), intent(in) :: walkers(*)
       real(c_double)                 :: E(*),Ec(*),Ep(*)
       integer(c_int) :: rc
     end function pigs_therm_energy_batch

     ! LocalEnergy (reference sample_mod.f90:154)
     function pigs_local_energy_batch(ctx,n,walkers,ib,E,Kin,Pot) bind(C,name='pigs_local_energy_batch') result(rc)
       import :: c_int, c_int32_t, c_double, c_ptr
       type(c_ptr), value             :: ctx
       integer(c_int32_t), value      :: n,ib
       integer(c_int32_t), intent(in) :: walkers(*)
       real(c_double)                 :: E(*),Kin(*),Pot(*)
       integer(c_int) :: rc
     end function pigs_local_energy_batch

     ! K6: device-resident sampler (diagonal sector, sampling='bis')
     function pigs_sampler_init(ctx,sp) bind(C,name='pigs_sampler_init') result(rc)
       import :: c_int, c_ptr, pigs_sweep_params
       type(c_ptr), value :: ctx
       type(pigs_sweep_params), intent(in) :: sp
       integer(c_int) :: rc
     end function pigs_sampler_init

     function pigs_sampler_set_rng(ctx,walker,mti,mt) bind(C,name='pigs_sampler_set_rng') result(rc)
       import :: c_int, c_int32_t, c_ptr
       type(c_ptr), value             :: ctx
       integer(c_int32_t), value      :: walker,mti
       integer(c_int32_t), intent(in) :: mt(0:623)
       integer(c_int) :: rc
     end function pigs_sampler_set_rng

     function pigs_sampler_get_rng(ctx,walker,mti,mt) bind(C,name='pigs_sampler_get_rng') result(rc)
       import :: c_int, c_int32_t, c_ptr
       type(c_ptr), value        :: ctx
       integer(c_int32_t), value :: walker
       integer(c_int32_t)        :: mti,mt(0:623)
       integer(c_int) :: rc
     end function pigs_sampler_get_rng

     function pigs_sampler_step(ctx,istep) bind(C,name='pigs_sampler_step') result(rc)
       import :: c_int, c_int32_t, c_ptr
       type(c_ptr), value        :: ctx
       integer(c_int32_t), value :: istep
       integer(c_int) :: rc
     end function pigs_sampler_step

     function pigs_sampler_counters(ctx,acc) bind(C,name='pigs_sampler_counters') result(rc)
       import :: c_int, c_int64_t, c_ptr
       type(c_ptr), value :: ctx
       integer(c_int64_t) :: acc(*)
       integer(c_int) :: rc
     end function pigs_sampler_counters

     ! (pigs_sampler_form is looked up at run time: see sampler_form below)
     function c_dlsym(handle,name) bind(C,name='dlsym') result(p)
       import :: c_ptr, c_funptr, c_char
       type(c_ptr), value :: handle
       character(kind=c_char), intent(in) :: name(*)
       type(c_funptr) :: p
     end function c_dlsym

     function pigs_sampler_counters16(ctx,cnt) bind(C,name='pigs_sampler_counters16') result(rc)
       import :: c_int, c_int64_t, c_ptr
       type(c_ptr), value :: ctx
       integer(c_int64_t) :: cnt(*)
       integer(c_int) :: rc
     end function pigs_sampler_counters16

     function pigs_sampler_get_worm(ctx,isopen,iworm,xend) bind(C,name='pigs_sampler_get_worm') result(rc)
       import :: c_int, c_int32_t, c_double, c_ptr
       type(c_ptr), value :: ctx
       integer(c_int32_t) :: isopen(*),iworm(*)
       real(c_double)     :: xend(*)
       integer(c_int) :: rc
     end function pigs_sampler_get_worm

     function pigs_sampler_set_worm(ctx,isopen,iworm,xend) bind(C,name='pigs_sampler_set_worm') result(rc)
       import :: c_int, c_int32_t, c_double, c_ptr
       type(c_ptr), value :: ctx
       integer(c_int32_t), intent(in) :: isopen(*),iworm(*)
       real(c_double), intent(in)     :: xend(*)
       integer(c_int) :: rc
     end function pigs_sampler_set_worm

     function pigs_sampler_events(ctx,events) bind(C,name='pigs_sampler_events') result(rc)
       import :: c_int, c_int32_t, c_ptr
       type(c_ptr), value :: ctx
       integer(c_int32_t) :: events(*)
       integer(c_int) :: rc
     end function pigs_sampler_events

     function pigs_sampler_nrho(ctx,nrho,reset) bind(C,name='pigs_sampler_nrho') result(rc)
       import :: c_int, c_int32_t, c_double, c_ptr
       type(c_ptr), value             :: ctx
       real(c_double)                 :: nrho(*)
       integer(c_int32_t), intent(in) :: reset(*)      ! per walker: 1 = zero the histogram after the copy
       integer(c_int) :: rc
     end function pigs_sampler_nrho

     function pigs_slice_download(ctx,ib,R) bind(C,name='pigs_slice_download') result(rc)
       import :: c_int, c_int32_t, c_double, c_ptr
       type(c_ptr), value        :: ctx
       integer(c_int32_t), value :: ib
       real(c_double)            :: R(*)
       integer(c_int) :: rc
     end function pigs_slice_download

     ! K7: PairCorrelation + StructureFactor increments of slice ib (reference sample_mod.f90:392-473)
     function pigs_structure_batch(ctx,n,walkers,ib,Nbin,rbin,Nk,gr,Sk) bind(C,name='pigs_structure_batch') result(rc)
       import :: c_int, c_int32_t, c_double, c_ptr
       type(c_ptr), value             :: ctx
       integer(c_int32_t), value      :: n,ib,Nbin,Nk
       integer(c_int32_t), intent(in) :: walkers(*)
       real(c_double), value          :: rbin
       real(c_double)                 :: gr(*),Sk(*)
       integer(c_int) :: rc
     end function pigs_structure_batch

     ! every estimator of a diagonal MC step in one call (reference vpi.f90:443-469): en(1:3,i) = LocalEnergy at slice 0,
     ! en(4:6,i) at slice 2Nb, en(7:9,i) = ThermEnergy of walker walkers(i); gr / Sk = c_null_ptr: no structural estimators
     function pigs_diagonal_estimators(ctx,n,walkers,Nbin,rbin,Nk,en,gr,Sk) bind(C,name='pigs_diagonal_estimators') result(rc)
       import :: c_int, c_int32_t, c_double, c_ptr
       type(c_ptr), value             :: ctx
       integer(c_int32_t), value      :: n,Nbin,Nk
       integer(c_int32_t), intent(in) :: walkers(*)
       real(c_double), value          :: rbin
       real(c_double)                 :: en(9,*)
       type(c_ptr), value             :: gr,Sk
       integer(c_int) :: rc
     end function pigs_diagonal_estimators

     ! the same overlapped with the next step of the device-resident sampler: _begin snapshots the worldlines and queues the
     ! estimator kernels on the context's second stream, _end collects (layouts as pigs_diagonal_estimators)
     function pigs_diagonal_estimators_begin(ctx,n,walkers,Nbin,rbin,Nk,structure) &
          & bind(C,name='pigs_diagonal_estimators_begin') result(rc)
       import :: c_int, c_int32_t, c_double, c_ptr
       type(c_ptr), value             :: ctx
       integer(c_int32_t), value      :: n,Nbin,Nk,structure
       integer(c_int32_t), intent(in) :: walkers(*)
       real(c_double), value          :: rbin
       integer(c_int) :: rc
     end function pigs_diagonal_estimators_begin

     function pigs_diagonal_estimators_end(ctx,en,gr,Sk) bind(C,name='pigs_diagonal_estimators_end') result(rc)
       import :: c_int, c_double, c_ptr
       type(c_ptr), value :: ctx
       real(c_double)     :: en(9,*)
       type(c_ptr), value :: gr,Sk
       integer(c_int) :: rc
     end function pigs_diagonal_estimators_end

     function pigs_sampler_event_ints(ctx,n) bind(C,name='pigs_sampler_event_ints') result(rc)
       import :: c_int, c_int32_t, c_ptr
       type(c_ptr), value :: ctx
       integer(c_int32_t) :: n
       integer(c_int) :: rc
     end function pigs_sampler_event_ints

     function pigs_comm_init_all(ctxs,nranks) bind(C,name='pigs_comm_init_all') result(rc)
       import :: c_int, c_int32_t, c_ptr
       type(c_ptr)               :: ctxs(*)
       integer(c_int32_t), value :: nranks
       integer(c_int) :: rc
     end function pigs_comm_init_all

     function pigs_estimators_allreduce(ctx,vec,n) bind(C,name='pigs_estimators_allreduce') result(rc)
       import :: c_int, c_int32_t, c_double, c_ptr
       type(c_ptr), value        :: ctx
       real(c_double)            :: vec(*)
       integer(c_int32_t), value :: n
       integer(c_int) :: rc
     end function pigs_estimators_allreduce

  end interface

  abstract interface
     function pigs_sampler_form_t(ctx,out) bind(C) result(rc)
       import :: c_int, c_int32_t, c_ptr
       type(c_ptr), value :: ctx
       integer(c_int32_t) :: out(4)
       integer(c_int) :: rc
     end function pigs_sampler_form_t

     ! pigs_*_accumulate of every estimator family: the slices of the walkers(1:n) (0-based) into the family's sums
     function pigs_accumulate_t(ctx,n,walkers) bind(C) result(rc)
       import :: c_int, c_int32_t, c_ptr
       type(c_ptr), value             :: ctx
       integer(c_int32_t), value      :: n
       integer(c_int32_t), intent(in) :: walkers(*)
       integer(c_int) :: rc
     end function pigs_accumulate_t

     ! density profiles of a trapped system (include/pigs_hip.h, pigs_density_*): looked up at run time, see density_bind
     function pigs_density_init_t(ctx,Nbin,half_width) bind(C) result(rc)
       import :: c_int, c_int32_t, c_double, c_ptr
       type(c_ptr), value        :: ctx
       integer(c_int32_t), value :: Nbin
       real(c_double), value     :: half_width
       integer(c_int) :: rc
     end function pigs_density_init_t

     function pigs_density_read_t(ctx,planar,radial,pair,samples,reset) bind(C) result(rc)
       import :: c_int, c_int32_t, c_int64_t, c_ptr
       type(c_ptr), value             :: ctx
       integer(c_int64_t)             :: planar(*),radial(*),pair(*),samples(*)
       integer(c_int32_t), intent(in) :: reset(*)      ! per walker: 1 = zero its accumulators after the copy
       integer(c_int) :: rc
     end function pigs_density_read_t

     ! imaginary-time density correlations of a periodic system (include/pigs_hip.h, pigs_fqt_*): looked up at run time,
     ! see fqt_bind
     function pigs_fqt_init_t(ctx,Nk,Ntau,window) bind(C) result(rc)
       import :: c_int, c_int32_t, c_ptr
       type(c_ptr), value        :: ctx
       integer(c_int32_t), value :: Nk,Ntau,window
       integer(c_int) :: rc
     end function pigs_fqt_init_t

     function pigs_fqt_read_t(ctx,F,samples,reset) bind(C) result(rc)
       import :: c_int, c_int32_t, c_int64_t, c_double, c_ptr
       type(c_ptr), value             :: ctx
       real(c_double)                 :: F(*)          ! raw sums (dim,Nk,0:Ntau,n_walkers)
       integer(c_int64_t)             :: samples(*)
       integer(c_int32_t), intent(in) :: reset(*)      ! per walker: 1 = zero its sums after the copy
       integer(c_int) :: rc
     end function pigs_fqt_read_t

     ! vector structure factor on the full reciprocal grid (include/pigs_hip.h, pigs_sqv_*): looked up at run time, see
     ! sqv_bind
     function pigs_sqv_init_t(ctx,nmax,window) bind(C) result(rc)
       import :: c_int, c_int32_t, c_ptr
       type(c_ptr), value        :: ctx
       integer(c_int32_t), value :: nmax,window
       integer(c_int) :: rc
     end function pigs_sqv_init_t

     function pigs_sqv_count_t(ctx,Nq) bind(C) result(rc)
       import :: c_int, c_int64_t, c_ptr
       type(c_ptr), value :: ctx
       integer(c_int64_t) :: Nq
       integer(c_int) :: rc
     end function pigs_sqv_count_t

     function pigs_sqv_vectors_t(ctx,n) bind(C) result(rc)
       import :: c_int, c_int32_t, c_ptr
       type(c_ptr), value :: ctx
       integer(c_int32_t) :: n(*)                      ! the stored vectors (dim,Nq)
       integer(c_int) :: rc
     end function pigs_sqv_vectors_t

     function pigs_sqv_read_t(ctx,S,samples,reset) bind(C) result(rc)
       import :: c_int, c_int32_t, c_int64_t, c_double, c_ptr
       type(c_ptr), value             :: ctx
       real(c_double)                 :: S(*)          ! raw sums (Nq,n_walkers)
       integer(c_int64_t)             :: samples(*)
       integer(c_int32_t), intent(in) :: reset(*)      ! per walker: 1 = zero its sums after the copy
       integer(c_int) :: rc
     end function pigs_sqv_read_t

     ! pair distribution on the vector grid over a slice window (include/pigs_hip.h, pigs_grv_*): looked up at run time,
     ! see grv_bind
     function pigs_grv_init_t(ctx,Nbin,Nr,rbin,window) bind(C) result(rc)
       import :: c_int, c_int32_t, c_double, c_ptr
       type(c_ptr), value        :: ctx
       integer(c_int32_t), value :: Nbin,Nr
       real(c_double), value     :: rbin
       integer(c_int32_t), value :: window
       integer(c_int) :: rc
     end function pigs_grv_init_t

     function pigs_grv_read_t(ctx,vec,radial,samples,reset) bind(C) result(rc)
       import :: c_int, c_int32_t, c_int64_t, c_ptr
       type(c_ptr), value             :: ctx
       integer(c_int64_t)             :: vec(*)        ! counts (Nbin**dim,n_walkers), x fastest
       integer(c_int64_t)             :: radial(*)     ! counts (Nr,n_walkers)
       integer(c_int64_t)             :: samples(*)
       integer(c_int32_t), intent(in) :: reset(*)      ! per walker: 1 = zero its counts after the copy
       integer(c_int) :: rc
     end function pigs_grv_read_t

     ! F(q,tau) on the full reciprocal grid (include/pigs_hip.h, pigs_fqv_*): looked up at run time, see fqv_bind; _count
     ! and _vectors have the signatures of the pigs_sqv_* ones
     function pigs_fqv_init_t(ctx,nmax,Ntau,window) bind(C) result(rc)
       import :: c_int, c_int32_t, c_ptr
       type(c_ptr), value        :: ctx
       integer(c_int32_t), value :: nmax,Ntau,window
       integer(c_int) :: rc
     end function pigs_fqv_init_t

     function pigs_fqv_read_t(ctx,F,samples,reset) bind(C) result(rc)
       import :: c_int, c_int32_t, c_int64_t, c_double, c_ptr
       type(c_ptr), value             :: ctx
       real(c_double)                 :: F(*)          ! raw sums (Nq,0:Ntau,n_walkers)
       integer(c_int64_t)             :: samples(*)
       integer(c_int32_t), intent(in) :: reset(*)      ! per walker: 1 = zero its sums after the copy
       integer(c_int) :: rc
     end function pigs_fqv_read_t

     ! self part of F(q,tau) and imaginary-time displacement (include/pigs_hip.h, pigs_fqs_*): looked up at run time, see
     ! fqs_bind; _init has the signature of pigs_fqv_init, _count and _vectors those of the pigs_sqv_* ones
     function pigs_fqs_read_t(ctx,F,D,samples,reset) bind(C) result(rc)
       import :: c_int, c_int32_t, c_int64_t, c_double, c_ptr
       type(c_ptr), value             :: ctx
       real(c_double)                 :: F(*)          ! raw sums (Nq,0:Ntau,n_walkers)
       real(c_double)                 :: D(*)          ! raw sums of r^2 and r^4 (2,0:Ntau,n_walkers)
       integer(c_int64_t)             :: samples(*)
       integer(c_int32_t), intent(in) :: reset(*)      ! per walker: 1 = zero its sums after the copy
       integer(c_int) :: rc
     end function pigs_fqs_read_t

     ! imaginary-time profiles (include/pigs_hip.h, pigs_tau_*): looked up at run time, see tau_bind
     function pigs_tau_init_t(ctx) bind(C) result(rc)
       import :: c_int, c_ptr
       type(c_ptr), value :: ctx
       integer(c_int) :: rc
     end function pigs_tau_init_t

     function pigs_tau_read_t(ctx,Q,samples,reset) bind(C) result(rc)
       import :: c_int, c_int32_t, c_int64_t, c_double, c_ptr
       type(c_ptr), value             :: ctx
       real(c_double)                 :: Q(*)          ! raw sums (4,0:2Nb,n_walkers): Vpair, Vext, W, D2
       integer(c_int64_t)             :: samples(*)
       integer(c_int32_t), intent(in) :: reset(*)      ! per walker: 1 = zero its sums after the copy
       integer(c_int) :: rc
     end function pigs_tau_read_t

     ! bond-orientational order over a slice window (include/pigs_hip.h, pigs_bop_*): looked up at run time, see bop_bind
     function pigs_bop_init_t(ctx,rnb,window,Nh,Nr,rbin) bind(C) result(rc)
       import :: c_int, c_int32_t, c_double, c_ptr
       type(c_ptr), value        :: ctx
       real(c_double), value     :: rnb
       integer(c_int32_t), value :: window,Nh,Nr
       real(c_double), value     :: rbin
       integer(c_int) :: rc
     end function pigs_bop_init_t

     function pigs_bop_read_t(ctx,S,H,G,GN,samples,reset) bind(C) result(rc)
       import :: c_int, c_int32_t, c_int64_t, c_double, c_ptr
       type(c_ptr), value             :: ctx
       real(c_double)                 :: S(*)          ! raw sums (8,n_walkers)
       integer(c_int64_t)             :: H(*)          ! counts (Nh,2,n_walkers)
       real(c_double)                 :: G(*)          ! raw sums (Nr,n_walkers)
       integer(c_int64_t)             :: GN(*)         ! pairs (Nr,n_walkers)
       integer(c_int64_t)             :: samples(*)
       integer(c_int32_t), intent(in) :: reset(*)      ! per walker: 1 = zero its sums after the copy
       integer(c_int) :: rc
     end function pigs_bop_read_t

     ! van Hove functions over a slice window (include/pigs_hip.h, pigs_vh_*): looked up at run time, see vh_bind
     function pigs_vh_init_t(ctx,Ntau,window,Nr,rbin,Ns,sbin) bind(C) result(rc)
       import :: c_int, c_int32_t, c_double, c_ptr
       type(c_ptr), value        :: ctx
       integer(c_int32_t), value :: Ntau,window,Nr
       real(c_double), value     :: rbin
       integer(c_int32_t), value :: Ns
       real(c_double), value     :: sbin
       integer(c_int) :: rc
     end function pigs_vh_init_t

     function pigs_vh_read_t(ctx,self,dist,samples,reset) bind(C) result(rc)
       import :: c_int, c_int32_t, c_int64_t, c_ptr
       type(c_ptr), value             :: ctx
       integer(c_int64_t)             :: self(*)       ! counts (Ns,Ntau+1,n_walkers)
       integer(c_int64_t)             :: dist(*)       ! counts (Nr,Ntau+1,n_walkers)
       integer(c_int64_t)             :: samples(*)
       integer(c_int32_t), intent(in) :: reset(*)      ! per walker: 1 = zero its counts after the copy
       integer(c_int) :: rc
     end function pigs_vh_read_t

     ! triplet distribution over a slice window (include/pigs_hip.h, pigs_g3_*): looked up at run time, see g3_bind
     function pigs_g3_init_t(ctx,Nr,rbin,Na,window) bind(C) result(rc)
       import :: c_int, c_int32_t, c_double, c_ptr
       type(c_ptr), value        :: ctx
       integer(c_int32_t), value :: Nr
       real(c_double), value     :: rbin
       integer(c_int32_t), value :: Na,window
       integer(c_int) :: rc
     end function pigs_g3_init_t

     function pigs_g3_read_t(ctx,trip,pair,samples,reset) bind(C) result(rc)
       import :: c_int, c_int32_t, c_int64_t, c_ptr
       type(c_ptr), value             :: ctx
       integer(c_int64_t)             :: trip(*)       ! counts (Na,Nr(Nr+1)/2,n_walkers)
       integer(c_int64_t)             :: pair(*)       ! counts (Nr,n_walkers)
       integer(c_int64_t)             :: samples(*)
       integer(c_int32_t), intent(in) :: reset(*)      ! per walker: 1 = zero its counts after the copy
       integer(c_int) :: rc
     end function pigs_g3_read_t

     ! Axilrod-Teller-Muto three-body sum over a slice window (include/pigs_hip.h, pigs_atm_*): looked up at run time, see
     ! atm_bind
     function pigs_atm_init_t(ctx,rc,window) bind(C) result(st)
       import :: c_int, c_int32_t, c_double, c_ptr
       type(c_ptr), value        :: ctx
       real(c_double), value     :: rc
       integer(c_int32_t), value :: window
       integer(c_int) :: st
     end function pigs_atm_init_t

     function pigs_atm_read_t(ctx,T,ntrip,samples,reset) bind(C) result(rc)
       import :: c_int, c_int32_t, c_int64_t, c_double, c_ptr
       type(c_ptr), value             :: ctx
       real(c_double)                 :: T(*)          ! raw sums (2 window + 1,n_walkers)
       integer(c_int64_t)             :: ntrip(*)      ! counts (2 window + 1,n_walkers)
       integer(c_int64_t)             :: samples(*)
       integer(c_int32_t), intent(in) :: reset(*)      ! per walker: 1 = zero its sums after the copy
       integer(c_int) :: rc
     end function pigs_atm_read_t

     ! momentum distribution and one-body density matrix (include/pigs_hip.h, pigs_nk_*): looked up at run time, see
     ! nk_bind; _init, _count and _vectors have the signatures of the pigs_sqv_* ones
     function pigs_nk_add_t(ctx,n,walkers,nsamp,xend) bind(C) result(rc)
       import :: c_int, c_int32_t, c_double, c_ptr
       type(c_ptr), value             :: ctx
       integer(c_int32_t), value      :: n
       integer(c_int32_t), intent(in) :: walkers(*),nsamp(*)
       real(c_double), intent(in)     :: xend(*)       ! (dim,2,sum nsamp): head, tail of every pair
       integer(c_int) :: rc
     end function pigs_nk_add_t

     function pigs_nk_read_t(ctx,C,H,nopen,ninside,reset) bind(C) result(rc)
       import :: c_int, c_int32_t, c_int64_t, c_double, c_ptr
       type(c_ptr), value             :: ctx
       real(c_double)                 :: C(*)          ! cosine sums (Nq,n_walkers)
       integer(c_int64_t)             :: H(*)          ! counts (nbin**dim,n_walkers)
       integer(c_int64_t)             :: nopen(*),ninside(*)
       integer(c_int32_t), intent(in) :: reset(*)      ! per walker: 1 = zero its sums after the copy
       integer(c_int) :: rc
     end function pigs_nk_read_t

     ! a crystal seen from its lattice (include/pigs_hip.h, pigs_lat_*): looked up at run time, see lat_bind
     function pigs_lat_init_t(ctx,nsite,sites,nbin,rmax,window,cm) bind(C) result(st)
       import :: c_int, c_int32_t, c_double, c_ptr
       type(c_ptr), value         :: ctx
       integer(c_int32_t), value  :: nsite,nbin,window,cm
       real(c_double), intent(in) :: sites(*)          ! R(dim,nsite)
       real(c_double), value      :: rmax
       integer(c_int) :: st
     end function pigs_lat_init_t

     function pigs_lat_read_t(ctx,mom,nassigned,nlost,occ,hr,hx,hop1,hopw,samples,reset) bind(C) result(rc)
       import :: c_int, c_int32_t, c_int64_t, c_double, c_ptr
       type(c_ptr), value             :: ctx
       real(c_double)                 :: mom(*)        ! (2+dim,2 window + 1,n_walkers)
       integer(c_int64_t)             :: nassigned(*)  ! (2 window + 1,n_walkers)
       integer(c_int64_t)             :: occ(*)        ! (4,2 window + 1,n_walkers)
       integer(c_int64_t)             :: hr(*),hx(*)   ! (nbin,n_walkers), (2 nbin,dim,n_walkers)
       integer(c_int64_t)             :: nlost(*),hop1(*),hopw(*),samples(*)
       integer(c_int32_t), intent(in) :: reset(*)      ! per walker: 1 = zero its sums after the copy
       integer(c_int) :: rc
     end function pigs_lat_read_t

     ! the superfluid fraction from the centre-of-mass diffusion along tau (include/pigs_hip.h, pigs_sf_*): looked up at
     ! run time, see sf_bind
     function pigs_sf_init_t(ctx,Ntau,window) bind(C) result(st)
       import :: c_int, c_int32_t, c_ptr
       type(c_ptr), value         :: ctx
       integer(c_int32_t), value  :: Ntau,window
       integer(c_int) :: st
     end function pigs_sf_init_t

     function pigs_sf_read_t(ctx,C,D,nwrap,samples,reset) bind(C) result(rc)
       import :: c_int, c_int32_t, c_int64_t, c_double, c_ptr
       type(c_ptr), value             :: ctx
       real(c_double)                 :: C(*),D(*)     ! (dim,0:Ntau,n_walkers)
       integer(c_int64_t)             :: nwrap(*),samples(*)
       integer(c_int32_t), intent(in) :: reset(*)      ! per walker: 1 = zero its sums after the copy
       integer(c_int) :: rc
     end function pigs_sf_read_t

     ! the cluster-size distribution over a slice window (include/pigs_hip.h, pigs_cl_*): looked up at run time, see
     ! cl_bind
     function pigs_cl_init_t(ctx,rc,window) bind(C) result(st)
       import :: c_int, c_int32_t, c_double, c_ptr
       type(c_ptr), value         :: ctx
       real(c_double), value      :: rc
       integer(c_int32_t), value  :: window
       integer(c_int) :: st
     end function pigs_cl_init_t

     function pigs_cl_read_t(ctx,nsize,nlarge,nbond,samples,rg2,reset) bind(C) result(rc)
       import :: c_int, c_int32_t, c_int64_t, c_double, c_ptr
       type(c_ptr), value             :: ctx
       integer(c_int64_t)             :: nsize(*),nlarge(*)     ! (Np,n_walkers)
       integer(c_int64_t)             :: nbond(*),samples(*)
       real(c_double)                 :: rg2(*)                 ! (Np,n_walkers)
       integer(c_int32_t), intent(in) :: reset(*)      ! per walker: 1 = zero its sums after the copy
       integer(c_int) :: rc
     end function pigs_cl_read_t

     ! wrapping clusters and cluster persistence over a slice window (include/pigs_hip.h, pigs_pc_*): looked up at run
     ! time, see pc_bind
     function pigs_pc_init_t(ctx,rc,window,ntau) bind(C) result(st)
       import :: c_int, c_int32_t, c_double, c_ptr
       type(c_ptr), value         :: ctx
       real(c_double), value      :: rc
       integer(c_int32_t), value  :: window,ntau
       integer(c_int) :: st
     end function pigs_pc_init_t

     function pigs_pc_read_t(ctx,nwrap,mwrap,swrap,nfin,samples,rg2u,first,second,both,norig,reset) bind(C) result(rc)
       import :: c_int, c_int32_t, c_int64_t, c_double, c_ptr
       type(c_ptr), value             :: ctx
       integer(c_int64_t)             :: nwrap(*),mwrap(*),swrap(*)        ! (8,n_walkers), index = wrap mask
       integer(c_int64_t)             :: nfin(*),samples(*)                ! (Np,n_walkers)
       real(c_double)                 :: rg2u(*)                           ! (Np,n_walkers)
       integer(c_int64_t)             :: first(*),second(*),both(*),norig(*)   ! (ntau+1,n_walkers)
       integer(c_int32_t), intent(in) :: reset(*)      ! per walker: 1 = zero its sums after the copy
       integer(c_int) :: rc
     end function pigs_pc_read_t
  end interface

  ! bound by density_bind (null until then)
  procedure(pigs_density_init_t), pointer       :: dens_init => null()
  procedure(pigs_accumulate_t), pointer         :: dens_accumulate => null()
  procedure(pigs_density_read_t), pointer       :: dens_read => null()

  ! bound by fqt_bind (null until then)
  procedure(pigs_fqt_init_t), pointer       :: fqt_init => null()
  procedure(pigs_accumulate_t), pointer     :: fqt_accumulate => null()
  procedure(pigs_fqt_read_t), pointer       :: fqt_read => null()

  ! bound by sqv_bind (null until then)
  procedure(pigs_sqv_init_t), pointer       :: sqv_init => null()
  procedure(pigs_sqv_count_t), pointer      :: sqv_count => null()
  procedure(pigs_sqv_vectors_t), pointer    :: sqv_vectors => null()
  procedure(pigs_accumulate_t), pointer     :: sqv_accumulate => null()
  procedure(pigs_sqv_read_t), pointer       :: sqv_read => null()

  ! bound by grv_bind (null until then)
  procedure(pigs_grv_init_t), pointer       :: grv_init => null()
  procedure(pigs_accumulate_t), pointer     :: grv_accumulate => null()
  procedure(pigs_grv_read_t), pointer       :: grv_read => null()

  ! bound by fqv_bind (null until then)
  procedure(pigs_fqv_init_t), pointer       :: fqv_init => null()
  procedure(pigs_sqv_count_t), pointer      :: fqv_count => null()
  procedure(pigs_sqv_vectors_t), pointer    :: fqv_vectors => null()
  procedure(pigs_accumulate_t), pointer     :: fqv_accumulate => null()
  procedure(pigs_fqv_read_t), pointer       :: fqv_read => null()

  ! bound by fqs_bind (null until then)
  procedure(pigs_fqv_init_t), pointer       :: fqs_init => null()
  procedure(pigs_sqv_count_t), pointer      :: fqs_count => null()
  procedure(pigs_sqv_vectors_t), pointer    :: fqs_vectors => null()
  procedure(pigs_accumulate_t), pointer     :: fqs_accumulate => null()
  procedure(pigs_fqs_read_t), pointer       :: fqs_read => null()

  ! bound by tau_bind (null until then)
  procedure(pigs_tau_init_t), pointer       :: tau_init => null()
  procedure(pigs_accumulate_t), pointer     :: tau_accumulate => null()
  procedure(pigs_tau_read_t), pointer       :: tau_read => null()

  ! bound by bop_bind (null until then)
  procedure(pigs_bop_init_t), pointer       :: bop_init => null()
  procedure(pigs_accumulate_t), pointer     :: bop_accumulate => null()
  procedure(pigs_bop_read_t), pointer       :: bop_read => null()

  ! bound by vh_bind (null until then)
  procedure(pigs_vh_init_t), pointer        :: vh_init => null()
  procedure(pigs_accumulate_t), pointer     :: vh_accumulate => null()
  procedure(pigs_vh_read_t), pointer        :: vh_read => null()

  ! bound by g3_bind (null until then)
  procedure(pigs_g3_init_t), pointer        :: g3_init => null()
  procedure(pigs_accumulate_t), pointer     :: g3_accumulate => null()
  procedure(pigs_g3_read_t), pointer        :: g3_read => null()

  ! bound by atm_bind (null until then)
  procedure(pigs_atm_init_t), pointer       :: atm_init => null()
  procedure(pigs_accumulate_t), pointer     :: atm_accumulate => null()
  procedure(pigs_atm_read_t), pointer       :: atm_read => null()

  ! bound by nk_bind (null until then)
  procedure(pigs_sqv_init_t), pointer       :: nk_init => null()
  procedure(pigs_sqv_count_t), pointer      :: nk_count => null()
  procedure(pigs_sqv_vectors_t), pointer    :: nk_vectors => null()
  procedure(pigs_accumulate_t), pointer     :: nk_accumulate => null()
  procedure(pigs_nk_add_t), pointer         :: nk_add => null()
  procedure(pigs_nk_read_t), pointer        :: nk_read => null()

  ! bound by lat_bind (null until then)
  procedure(pigs_lat_init_t), pointer       :: lat_init => null()
  procedure(pigs_accumulate_t), pointer     :: lat_accumulate => null()
  procedure(pigs_lat_read_t), pointer       :: lat_read => null()

  ! bound by sf_bind (null until then)
  procedure(pigs_sf_init_t), pointer        :: sf_init => null()
  procedure(pigs_accumulate_t), pointer     :: sf_accumulate => null()
  procedure(pigs_sf_read_t), pointer        :: sf_read => null()

  ! bound by cl_bind (null until then)
  procedure(pigs_cl_init_t), pointer        :: cl_init => null()
  procedure(pigs_accumulate_t), pointer     :: cl_accumulate => null()
  procedure(pigs_cl_read_t), pointer        :: cl_read => null()

  ! bound by pc_bind (null until then)
  procedure(pigs_pc_init_t), pointer        :: pc_init => null()
  procedure(pigs_accumulate_t), pointer     :: pc_accumulate => null()
  procedure(pigs_pc_read_t), pointer        :: pc_read => null()

contains

  ! pigs_sampler_form (the kernel form the device-resident sampler ran in) where the backend exports it: a report, not
  ! a dependency -- found at run time in the process's libraries (dlsym with RTLD_DEFAULT = NULL), so the host still links
  ! against backends without it.  .false. where it is not there.
  logical function sampler_form(ctx,form)
    type(c_ptr), intent(in)         :: ctx
    integer(c_int32_t), intent(out) :: form(4)
    type(c_funptr) :: f
    procedure(pigs_sampler_form_t), pointer :: query
    form = 0
    f = c_dlsym(c_null_ptr,'pigs_sampler_form'//c_null_char)
    sampler_form = c_associated(f)
    if (.not. sampler_form) return
    call c_f_procpointer(f,query)
    call pigs_check(query(ctx,form),'pigs_sampler_form')
  end function sampler_form

  ! The entry points pre_names(1), pre_names(2), ... looked up in the process's libraries (dlsym with RTLD_DEFAULT = NULL):
  ! .true. where every one is there.
  logical function resolve_all(pre,names,f)
    character(len=*), intent(in) :: pre,names(:)
    type(c_funptr), intent(out)  :: f(size(names))
    integer :: i
    resolve_all = .true.
    do i=1,size(names)
       f(i) = c_dlsym(c_null_ptr,pre//'_'//trim(names(i))//c_null_char)
       resolve_all = resolve_all .and. c_associated(f(i))
    end do
  end function resolve_all

  ! The density-profile entry points, found at run time and only when a run asks for them: the host links against
  ! backends without them (the CPU twin of tests/shim) and never names them at link time.  .false. (pointers left null)
  ! where the backend does not export all three.
  logical function density_bind()
    type(c_funptr) :: f(3)
    density_bind = resolve_all('pigs_density',[character(len=10) :: 'init','accumulate','read'],f)
    if (.not. density_bind) return
    call c_f_procpointer(f(1),dens_init)
    call c_f_procpointer(f(2),dens_accumulate)
    call c_f_procpointer(f(3),dens_read)
  end function density_bind

  ! The F(q,tau) entry points, found like the density ones: at run time, only when a run asks for them.
  logical function fqt_bind()
    type(c_funptr) :: f(3)
    fqt_bind = resolve_all('pigs_fqt',[character(len=10) :: 'init','accumulate','read'],f)
    if (.not. fqt_bind) return
    call c_f_procpointer(f(1),fqt_init)
    call c_f_procpointer(f(2),fqt_accumulate)
    call c_f_procpointer(f(3),fqt_read)
  end function fqt_bind

  ! The vector-S(q) entry points, found like the F(q,tau) ones: at run time, only when a run asks for them.
  logical function sqv_bind()
    type(c_funptr) :: f(5)
    sqv_bind = resolve_all('pigs_sqv',[character(len=10) :: 'init','count','vectors','accumulate','read'],f)
    if (.not. sqv_bind) return
    call c_f_procpointer(f(1),sqv_init)
    call c_f_procpointer(f(2),sqv_count)
    call c_f_procpointer(f(3),sqv_vectors)
    call c_f_procpointer(f(4),sqv_accumulate)
    call c_f_procpointer(f(5),sqv_read)
  end function sqv_bind

  ! The vector-g(r) entry points, found like the vector-S(q) ones: at run time, only when a run asks for them.
  logical function grv_bind()
    type(c_funptr) :: f(3)
    grv_bind = resolve_all('pigs_grv',[character(len=10) :: 'init','accumulate','read'],f)
    if (.not. grv_bind) return
    call c_f_procpointer(f(1),grv_init)
    call c_f_procpointer(f(2),grv_accumulate)
    call c_f_procpointer(f(3),grv_read)
  end function grv_bind

  ! The vector-F(q,tau) entry points, found like the vector-S(q) ones: at run time, only when a run asks for them.
  logical function fqv_bind()
    type(c_funptr) :: f(5)
    fqv_bind = resolve_all('pigs_fqv',[character(len=10) :: 'init','count','vectors','accumulate','read'],f)
    if (.not. fqv_bind) return
    call c_f_procpointer(f(1),fqv_init)
    call c_f_procpointer(f(2),fqv_count)
    call c_f_procpointer(f(3),fqv_vectors)
    call c_f_procpointer(f(4),fqv_accumulate)
    call c_f_procpointer(f(5),fqv_read)
  end function fqv_bind

  ! The entry points of the self part of F(q,tau), found like the vector-F(q,tau) ones: at run time, only when a run asks
  ! for them.
  logical function fqs_bind()
    type(c_funptr) :: f(5)
    fqs_bind = resolve_all('pigs_fqs',[character(len=10) :: 'init','count','vectors','accumulate','read'],f)
    if (.not. fqs_bind) return
    call c_f_procpointer(f(1),fqs_init)
    call c_f_procpointer(f(2),fqs_count)
    call c_f_procpointer(f(3),fqs_vectors)
    call c_f_procpointer(f(4),fqs_accumulate)
    call c_f_procpointer(f(5),fqs_read)
  end function fqs_bind

  ! The imaginary-time-profile entry points, found like the F(q,tau) ones: at run time, only when a run asks for them.
  logical function tau_bind()
    type(c_funptr) :: f(3)
    tau_bind = resolve_all('pigs_tau',[character(len=10) :: 'init','accumulate','read'],f)
    if (.not. tau_bind) return
    call c_f_procpointer(f(1),tau_init)
    call c_f_procpointer(f(2),tau_accumulate)
    call c_f_procpointer(f(3),tau_read)
  end function tau_bind

  ! The bond-orientational-order entry points, found like the F(q,tau) ones: at run time, only when a run asks for them.
  logical function bop_bind()
    type(c_funptr) :: f(3)
    bop_bind = resolve_all('pigs_bop',[character(len=10) :: 'init','accumulate','read'],f)
    if (.not. bop_bind) return
    call c_f_procpointer(f(1),bop_init)
    call c_f_procpointer(f(2),bop_accumulate)
    call c_f_procpointer(f(3),bop_read)
  end function bop_bind

  ! The van Hove entry points, found like the F(q,tau) ones: at run time, only when a run asks for them.
  logical function vh_bind()
    type(c_funptr) :: f(3)
    vh_bind = resolve_all('pigs_vh',[character(len=10) :: 'init','accumulate','read'],f)
    if (.not. vh_bind) return
    call c_f_procpointer(f(1),vh_init)
    call c_f_procpointer(f(2),vh_accumulate)
    call c_f_procpointer(f(3),vh_read)
  end function vh_bind

  ! The triplet entry points, found like the F(q,tau) ones: at run time, only when a run asks for them.
  logical function g3_bind()
    type(c_funptr) :: f(3)
    g3_bind = resolve_all('pigs_g3',[character(len=10) :: 'init','accumulate','read'],f)
    if (.not. g3_bind) return
    call c_f_procpointer(f(1),g3_init)
    call c_f_procpointer(f(2),g3_accumulate)
    call c_f_procpointer(f(3),g3_read)
  end function g3_bind

  ! The three-body entry points, found like the F(q,tau) ones: at run time, only when a run asks for them.
  logical function atm_bind()
    type(c_funptr) :: f(3)
    atm_bind = resolve_all('pigs_atm',[character(len=10) :: 'init','accumulate','read'],f)
    if (.not. atm_bind) return
    call c_f_procpointer(f(1),atm_init)
    call c_f_procpointer(f(2),atm_accumulate)
    call c_f_procpointer(f(3),atm_read)
  end function atm_bind

  ! The momentum-distribution entry points, found like the F(q,tau) ones: at run time, only when a run asks for them.
  logical function nk_bind()
    type(c_funptr) :: f(6)
    nk_bind = resolve_all('pigs_nk',[character(len=10) :: 'init','count','vectors','accumulate','add','read'],f)
    if (.not. nk_bind) return
    call c_f_procpointer(f(1),nk_init)
    call c_f_procpointer(f(2),nk_count)
    call c_f_procpointer(f(3),nk_vectors)
    call c_f_procpointer(f(4),nk_accumulate)
    call c_f_procpointer(f(5),nk_add)
    call c_f_procpointer(f(6),nk_read)
  end function nk_bind

  ! The lattice entry points, found like the F(q,tau) ones: at run time, only when a run asks for them.
  logical function lat_bind()
    type(c_funptr) :: f(3)
    lat_bind = resolve_all('pigs_lat',[character(len=10) :: 'init','accumulate','read'],f)
    if (.not. lat_bind) return
    call c_f_procpointer(f(1),lat_init)
    call c_f_procpointer(f(2),lat_accumulate)
    call c_f_procpointer(f(3),lat_read)
  end function lat_bind

  ! The centre-of-mass diffusion entry points, found like the F(q,tau) ones: at run time, only when a run asks for them.
  logical function sf_bind()
    type(c_funptr) :: f(3)
    sf_bind = resolve_all('pigs_sf',[character(len=10) :: 'init','accumulate','read'],f)
    if (.not. sf_bind) return
    call c_f_procpointer(f(1),sf_init)
    call c_f_procpointer(f(2),sf_accumulate)
    call c_f_procpointer(f(3),sf_read)
  end function sf_bind

  ! The cluster entry points, found like the F(q,tau) ones: at run time, only when a run asks for them.
  logical function cl_bind()
    type(c_funptr) :: f(3)
    cl_bind = resolve_all('pigs_cl',[character(len=10) :: 'init','accumulate','read'],f)
    if (.not. cl_bind) return
    call c_f_procpointer(f(1),cl_init)
    call c_f_procpointer(f(2),cl_accumulate)
    call c_f_procpointer(f(3),cl_read)
  end function cl_bind

  ! The percolation entry points, found like the F(q,tau) ones: at run time, only when a run asks for them.
  logical function pc_bind()
    type(c_funptr) :: f(3)
    pc_bind = resolve_all('pigs_pc',[character(len=10) :: 'init','accumulate','read'],f)
    if (.not. pc_bind) return
    call c_f_procpointer(f(1),pc_init)
    call c_f_procpointer(f(2),pc_accumulate)
    call c_f_procpointer(f(3),pc_read)
  end function pc_bind

  ! Stop with the library's error text: the host-side policy (the library itself never stops).
  subroutine pigs_check(rc,what)
    integer(c_int), intent(in)   :: rc
    character(len=*), intent(in) :: what
    character(kind=c_char), pointer :: s(:)
    type(c_ptr) :: p
    integer :: n
    if (rc==PIGS_OK) return
    p = pigs_last_error()
    write (0,'(a,a,a,i0)') 'pigs: ',what,' failed with status ',rc
    if (c_associated(p)) then
       call c_f_pointer(p,s,[512])
       n = 1
       do while (n<512 .and. s(n)/=c_null_char)
          n = n+1
       end do
       write (0,'(512a1)') s(1:n-1)
    end if
    stop 1
  end subroutine pigs_check

end module pigs_capi
