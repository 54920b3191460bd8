// Factories for the native models, shaped like the reference's NeuralCodecs.Create{SNAC,DAC,Encodec}Async (NeuralCodecs.Torch/
// NeuralCodecs.cs:38-80: same parameter lists; the reference class is `public static partial class NeuralCodecs`, so these members
// join it), the tensor <-> host-array marshalling the *Native models use at their TorchSharp-typed API surface, and NcSession, the
// incremental session DACNative / SNACNative hand out (DecodeSession / EncodeSession), and NcSessionPool, the pool of independent streams
// they hand out (DecodePool / EncodePool).
// `path` names an NCWB weight blob (tools/convert_checkpoint.py converts HF safetensors / Descript .pth / SNAC torch files).
using System;
using System.IO;
using System.Threading.Tasks;
using NeuralCodecs.Core;
using NeuralCodecs.Core.Configuration;
using NeuralCodecs.Core.Exceptions;
using NeuralCodecs.Core.Loading;
using NeuralCodecs.Torch.Config.DAC;
using NeuralCodecs.Torch.Config.Encodec;
using NeuralCodecs.Torch.Config.SNAC;
using NeuralCodecs.Torch.Models;
using NeuralCodecs.Torch.Native;
using TorchSharp;
using static TorchSharp.torch;

namespace NeuralCodecs.Torch;

public static partial class NeuralCodecs
{
    public static Task<SNACNative> CreateSNACNativeAsync(string path, SNACConfig? config = null, ModelLoadOptions? options = null)   // NeuralCodecs.cs:38-44
    {
        return LoadNative(path, options, device =>
        {
            config ??= new SNACConfig();
            if (device is not null) config.Device = device;
            return new SNACNative(config);
        });
    }

    public static Task<DACNative> CreateDACNativeAsync(string path, DACConfig? config = null, ModelLoadOptions? options = null)      // NeuralCodecs.cs:56-63
    {
        return LoadNative(path, options, device =>
        {
            config ??= new DACConfig();
            if (device is not null) config.Device = device;
            return new DACNative(config);
        });
    }

    public static Task<EncodecNative> CreateEncodecNativeAsync(string path, EncodecConfig? config = null, ModelLoadOptions? options = null)   // NeuralCodecs.cs:74-80
    {
        return LoadNative(path, options, device =>
        {
            config ??= new EncodecConfig();
            if (device is not null) config.Device = device;
            return new EncodecNative(config);
        });
    }

    // TorchModelLoader.LoadLocalModel (TorchModelLoader.cs:360-384): missing file -> LoadException; any other failure is wrapped
    // in a LoadException; the weights are read on a pool thread (TorchModelLoader.cs:488-492).
    private static Task<TModel> LoadNative<TModel>(string path, ModelLoadOptions? options, Func<DeviceConfiguration?, TModel> create)
        where TModel : class, INeuralCodec
    {
        if (string.IsNullOrEmpty(path)) throw new ArgumentException("Model path cannot be empty", nameof(path));
        return Task.Run(() =>
        {
            if (!File.Exists(path)) throw new LoadException($"Model file not found at {path}");
            TModel? model = null;
            try
            {
                model = create(options?.Device);
                model.LoadWeights(path);
                return model;
            }
            catch (Exception ex) when (ex is not LoadException)
            {
                model?.Dispose();
                throw new LoadException($"Failed to load local model: {path}. {ex.Message}", ex);
            }
        });
    }
}

/// <summary>Tensor <-> host array marshalling; only calls the reference itself makes on TorchSharp (DAC.cs:213-223, SNAC.cs:185).</summary>
internal static class NcTensor
{
    public static float[] Floats(Tensor t) => t.cpu().detach().to(torch.float32).contiguous().data<float>().ToArray();
    public static long[] Longs(Tensor t) => t.cpu().detach().to(torch.int64).contiguous().data<long>().ToArray();
    public static Tensor From(float[] a, params long[] shape) => torch.tensor(a, dtype: torch.float32).reshape(shape);
    public static Tensor From(long[] a, params long[] shape) => torch.tensor(a, dtype: torch.int64).reshape(shape);
}

/// <summary>An incremental session on a DAC or SNAC model (nc_session_*, include/nc_mi355x.h "incremental sessions"): codes or PCM are
/// pushed as they arrive and every call returns the outputs that became final; concatenated along time they are what the one-shot call
/// on the whole sequence returns, bit for bit.  Host arrays, synchronous.  The model must outlive its sessions.</summary>
public sealed unsafe class NcSession : IDisposable
{
    private IntPtr _s;
    private readonly int _rows;             // rows of an output: B (PCM, SNAC codes) or B * codebooks (DAC codes)

    internal NcSession(IntPtr session, int rows) { _s = session; _rows = rows; }

    /// <summary>Frames pushed and not yet emitted.</summary>
    public long Pending
    {
        get { long n; NcMi355x.Check(NcMi355x.nc_session_pending(_s, &n)); return n; }
    }

    /// <summary>After a reset the session is as new: the next push starts another clip.</summary>
    public void Reset() => NcMi355x.Check(NcMi355x.nc_session_reset(_s));

    /// <summary>Seed of the noise a SNAC decode session draws when a push carries none (not the draw of SNAC.Decode).</summary>
    public void SetSeed(ulong seed) => NcMi355x.Check(NcMi355x.nc_session_set_seed(_s, seed));

    /// <summary>Decode session: the next frames' codes (DAC [B,nQ,n]; SNAC the levels of a row side by side) -> PCM [B,nOut].</summary>
    public float[] PushCodes(long[] codes, long frames, float[]? noise, out long nOut)
    {
        ArgumentNullException.ThrowIfNull(codes);
        long cap, n;
        NcMi355x.Check(NcMi355x.nc_session_query(_s, frames, &cap));
        var buf = new float[_rows * Math.Max(cap, 1)];
        fixed (long* pc = codes) fixed (float* pn = noise, po = buf)
            NcMi355x.Check(NcMi355x.nc_session_push(_s, pc, frames, pn, po, cap, &n));
        nOut = n;
        return Rows(buf, cap, n);
    }

    /// <summary>Encode session: the next samples [B,n] -> codes (DAC [B,codebooks,nOut]; SNAC [B,nOut], the levels side by side).</summary>
    public long[] PushAudio(float[] pcm, long samples, out long nOut)
    {
        ArgumentNullException.ThrowIfNull(pcm);
        long cap, n;
        NcMi355x.Check(NcMi355x.nc_session_query(_s, samples, &cap));
        var buf = new long[_rows * Math.Max(cap, 1)];
        fixed (float* pp = pcm) fixed (long* po = buf)
            NcMi355x.Check(NcMi355x.nc_session_push(_s, pp, samples, null, po, cap, &n));
        nOut = n;
        return Rows(buf, cap, n);
    }

    /// <summary>The end of the clip of a decode session: everything not yet emitted.</summary>
    public float[] FlushAudio(out long nOut)
    {
        long cap, n;
        NcMi355x.Check(NcMi355x.nc_session_query(_s, 0, &cap));
        var buf = new float[_rows * Math.Max(cap, 1)];
        fixed (float* po = buf)
            NcMi355x.Check(NcMi355x.nc_session_flush(_s, po, cap, &n));
        nOut = n;
        return Rows(buf, cap, n);
    }

    /// <summary>The end of the clip of an encode session: the codes of the frames not yet emitted.</summary>
    public long[] FlushCodes(out long nOut)
    {
        long cap, n;
        NcMi355x.Check(NcMi355x.nc_session_query(_s, 0, &cap));
        var buf = new long[_rows * Math.Max(cap, 1)];
        fixed (long* po = buf)
            NcMi355x.Check(NcMi355x.nc_session_flush(_s, po, cap, &n));
        nOut = n;
        return Rows(buf, cap, n);
    }

    private T[] Rows<T>(T[] buf, long cap, long n)                                  // [rows, cap] -> dense [rows, n]
    {
        var dense = new T[_rows * n];
        for (int r = 0; r < _rows; ++r) Array.Copy(buf, r * cap, dense, r * n, n);
        return dense;
    }

    public void Dispose()
    {
        if (_s != IntPtr.Zero) { NcMi355x.nc_session_destroy(_s); _s = IntPtr.Zero; }
        GC.SuppressFinalize(this);
    }

    ~NcSession() { if (_s != IntPtr.Zero) NcMi355x.nc_session_destroy(_s); }
}

/// <summary>A session pool on a DAC or SNAC model (nc_session_pool_*, include/nc_mi355x.h "session pool"): independent streams in slots,
/// any subset of them advanced by one Step, each by its own amount; every slot returns what a single-row NcSession returns for the same
/// pushes, bit for bit.  Host arrays, synchronous.  The model must outlive its pools.</summary>
public sealed unsafe class NcSessionPool : IDisposable
{
    private IntPtr _p;
    private readonly int _outRows;          // rows of a slot's output: 1 (PCM, SNAC codes) or the codebooks (DAC codes)

    internal NcSessionPool(IntPtr pool, int outRows) { _p = pool; _outRows = outRows; }

    /// <summary>Frames the slot has pushed and not yet emitted.</summary>
    public long Pending(int slot)
    {
        long n;
        NcMi355x.Check(NcMi355x.nc_session_pool_pending(_p, slot, &n));
        return n;
    }

    /// <summary>After a reset the slot is as new: its next push starts another clip.</summary>
    public void Reset(int slot) => NcMi355x.Check(NcMi355x.nc_session_pool_reset_slot(_p, slot));

    /// <summary>Seed of the noise the slot of a SNAC decode pool draws when a step carries none: as NcSession.SetSeed for that stream.</summary>
    public void SetSeed(int slot, ulong seed) => NcMi355x.Check(NcMi355x.nc_session_pool_set_seed(_p, slot, seed));

    /// <summary>The exact outputs per row every entry of such a step would return now (nIn[i] == 0: a flush).</summary>
    public long[] Query(int[] slots, long[] nIn)
    {
        ArgumentNullException.ThrowIfNull(slots);
        ArgumentNullException.ThrowIfNull(nIn);
        if (nIn.Length != slots.Length) throw new ArgumentException("one nIn per slot");
        var nOut = new long[Math.Max(slots.Length, 1)];
        fixed (int* ps = slots) fixed (long* pi = nIn, po = nOut)
            NcMi355x.Check(NcMi355x.nc_session_pool_query(_p, slots.Length, ps, pi, po));
        return nOut;
    }

    /// <summary>Decode pool: entry i pushes nIn[i] frames of slot slots[i] (0: flush); codes packed entry after entry (DAC [nQ,n]; SNAC
    /// the levels side by side) -> PCM packed entry after entry, nOut[i] samples each.</summary>
    public float[] StepCodes(int[] slots, long[] nIn, long[]? codesPacked, float[]? noisePacked, out long[] nOut)
    {
        nOut = Query(slots, nIn);
        long cap = 0;
        for (int i = 0; i < slots.Length; ++i) cap += _outRows * nOut[i];
        var buf = new float[Math.Max(cap, 1)];
        fixed (int* ps = slots) fixed (long* pi = nIn, pc = codesPacked, pn = nOut) fixed (float* pz = noisePacked, po = buf)
            NcMi355x.Check(NcMi355x.nc_session_pool_step(_p, slots.Length, ps, pi, pc, pz, po, cap, pn));
        return buf.AsSpan(0, (int)cap).ToArray();
    }

    /// <summary>Encode pool: entry i pushes nIn[i] samples of slot slots[i] (0: flush); PCM packed entry after entry -> codes packed entry
    /// after entry (DAC [codebooks,nOut[i]]; SNAC the nOut[i] values of the emitted frames, levels side by side).</summary>
    public long[] StepAudio(int[] slots, long[] nIn, float[]? pcmPacked, out long[] nOut)
    {
        nOut = Query(slots, nIn);
        long cap = 0;
        for (int i = 0; i < slots.Length; ++i) cap += _outRows * nOut[i];
        var buf = new long[Math.Max(cap, 1)];
        fixed (int* ps = slots) fixed (long* pi = nIn, pn = nOut, po = buf) fixed (float* pp = pcmPacked)
            NcMi355x.Check(NcMi355x.nc_session_pool_step(_p, slots.Length, ps, pi, pp, null, po, cap, pn));
        return buf.AsSpan(0, (int)cap).ToArray();
    }

    public void Dispose()
    {
        if (_p != IntPtr.Zero) { NcMi355x.nc_session_pool_destroy(_p); _p = IntPtr.Zero; }
        GC.SuppressFinalize(this);
    }

    ~NcSessionPool() { if (_p != IntPtr.Zero) NcMi355x.nc_session_pool_destroy(_p); }
}
