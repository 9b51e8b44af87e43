// Host-side mirror of the reference's `fhe` package: the server half (fhe/bfv.go, fhe/code.go,
// fhe/ntt.go, fhe/ligero.go:19-370,638-705,755-797) and the client's ClientBFV, EncryptedProof.Decrypt and
// Proof.Verify (fhe/bfv.go:60-106, fhe/ligero.go:381-502,517-574), written above the C ABI of
// include/lumenos_hip.h.  Names, argument meaning and error behaviour follow the Go code so that a
// test written against it reads like fhe/ligero_test.go; where the Go code hands []*rlwe.Ciphertext
// around, this mirror hands `Ciphertexts` (an HBM-resident lumen_set) around.
#pragma once
#include <array>
#include <atomic>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/lumenos_hip.h"
#include "core.hpp"

namespace lumenos {
namespace vdec {
// The arguments of lazer's ProveVdecLnpTbox as vdec.CallVdecProver prepares them (vdec/prover.go:104-119,
// core/utils.go:12-33): centred coefficient vectors of the level-0 batch ciphertext, of the secret key and of the
// batched message at the ciphertext's scale, N entries each.  The reference hands lazer the first Degree of them
// (prover.go:92,138-143); the caller slices.  err = ct0 + ct1 * sk - mDelta mod q_0, centred: the e whose smallness
// lazer proves (the decryption is right exactly when |err| * 2T < q_0).
// Recorded deviation: prover.go:119 reads the NTT-domain words of the plaintext as if they were coefficients
// (isNTT = false); mDelta here is in the coefficient domain, like ct0 and ct1.
struct Witness {
    std::vector<int8_t> sk;
    std::vector<int64_t> ct0, ct1, mDelta, err;
    int Degree = 2048;
};
} // namespace vdec

namespace fhe {

// bgv.ParametersLiteral as produced by GenerateBGVParamsForNTT
struct ParametersLiteral {
    int LogN = 0;
    std::vector<int> LogQ, LogP;
    uint64_t PlaintextModulus = 0;
};

// fhe.GenerateBGVParamsForNTT (fhe/bfv.go:121-188); errors become std::invalid_argument with the
// reference's messages
ParametersLiteral GenerateBGVParamsForNTT(int nttSize, int logN, uint64_t plaintextModulus);

// the part of bgv.Parameters the path needs
struct Parameters {
    int LogN = 0;
    std::vector<uint64_t> Q, P;
    std::vector<uint64_t> Psi; // primitive 2N-th root per modulus (Q then P)
    uint64_t T = 0;
    int N() const { return 1 << LogN; }
    int MaxLevel() const { return (int)Q.size() - 1; }
    uint64_t PlaintextModulus() const { return T; }
    // bgv.NewParametersFromLiteral: [LATTIGO-RECALL] NTT-friendly primes nearest 2^bits, upstream first
    static Parameters FromLiteral(const ParametersLiteral &lit);
    // explicit moduli (what a Go host passes: Lattigo's own)
    static Parameters FromModuli(int logN, std::vector<uint64_t> q, std::vector<uint64_t> p, uint64_t T);
    uint64_t GaloisElement(int k) const; // 5^k mod 2N
    uint64_t GaloisElementForRowRotation() const { return (2ull << LogN) - 1; }
    // params.GaloisElementsForInnerSum(batch, n) (fhe/ligero_test.go:53, cmd/client/main.go:81): the elements
    // the CLIENT generates keys for -- rotations {1, 2, ..., n/2, n}*batch plus the row swap iff n > N/2
    // (12 / 14 / 15 / 16 keys at the four reference configurations, as their key-size logs show)
    std::vector<uint64_t> GaloisElementsForInnerSum(int batch, int n) const;
    // the subset InnerSum(ct, 1, n) applies, in the order it applies them (lumen_inner_sum_galois_elements)
    std::vector<uint64_t> GaloisElementsUsedByInnerSum(int n) const;
};

struct Plaintext { // *rlwe.Plaintext: one polynomial, NTT domain, [level+1][N]
    std::vector<uint64_t> Value;
    int Level = 0;
    uint64_t Scale = 1; // MetaData.Scale modulo T: Encoder.Encode of unscaled values leaves 1
};

class ServerBFV;
class ClientBFV;
class RingSwitchServer;
struct Proof;

// What a client posts to /keys (cmd/client/main.go:74-81, 124-131) before it is marshalled: the public key and one
// Galois key per entry of params.GaloisElementsForInnerSum(1, rows), in that order (rotations by N/2 and by N both
// map to the element 1, so an element may appear twice, with the same key).  Flags: 0 = standard-form words,
// LUMEN_KEY_MONTGOMERY = Lattigo's storage form (x * 2^64 mod q_i), what rlwe.GaloisKey holds.  Rlk: the
// relinearisation key of the same body (kgen.GenRelinearizationKeyNew, main.go:78), empty when the set carries none.
struct KeySet {
    std::vector<uint64_t> Pk;                      // [2][L+K][N]
    std::vector<uint64_t> GaloisElements;          // GaloisElementsForInnerSum(1, rows)
    std::vector<std::vector<uint64_t>> GaloisKeys; // [beta][b|a][L+K][N] each
    std::vector<uint64_t> Rlk;                     // [beta][b|a][L+K][N], or empty
    uint32_t Flags = 0;
};

// The same body in SEEDED form (include/lumenos_hip.h, "seeded switching keys"): every switching key travels as its b
// half, [beta][L+K][N], and the whole set shares ONE public 32-byte seed from which the server draws the `a` halves
// (lumen_load_galois_key_seeded / lumen_load_relin_key_seeded) -- half of cmd/client/main.go:74-81's upload.  ASeed is
// the ONE public seed of the client's keygen seed (ClientBFV::PublicKeySeed: drawn with it from getrandom(2), never equal
// to it, the same in every set that client generates): a key published under two different `a` gives its secret away
// (b1 - b2 = (a2 - a1) * s_out), so a client's keys never meet a second one.  The public key travels whole.  No wire format is defined for this struct.
struct SeededKeySet {
    std::array<uint8_t, 32> ASeed{};
    std::vector<uint64_t> Pk;                          // [2][L+K][N], or empty (a set of switching keys alone)
    std::map<uint64_t, std::vector<uint64_t>> GaloisB; // element -> [beta][L+K][N]
    std::vector<uint64_t> RlkB;                        // [beta][L+K][N], or empty
    uint32_t Flags = 0;                                // the form of the b words
};

// rlwe.MetaData of the ciphertexts of one slice (they are produced by the same calls, so they share it):
// what the Go shim's download() has to write into every rlwe.Ciphertext it materialises (SURVEY 8b,
// "Ownership").  Scale is bgv's plaintext scale modulo T: 1 after EncryptNew, multiplied by the
// plaintext's scale in MulNew and by q_l^-1 mod T for every limb Rescale drops.
struct MetaData {
    uint64_t Scale = 1;
    bool IsNTT = true, IsMontgomery = false, IsBatched = true;
    int LogRows = 1, LogCols = 0; // LogDimensions of the 2 x N/2 slot matrix
};

// The one owner of a lumen_ctx in this mirror: ServerBFV, ClientBFV and the plain backend of LigeroProveReference /
// EncodeRows each hold one.  It creates the context, records its ring degree (the C ABI does not give it back; what
// Ciphertexts::Download and the wire format size their buffers by) and destroys it, so an owner whose constructor
// throws half-way leaves nothing on the device.  Move-only.
class OwnedContext {
  public:
    OwnedContext() = default;
    OwnedContext(const Parameters &params, int device); // lumen_ctx_create of `params`
    // the plain context: ring degree 2^logN, the one modulus T (T = 1 mod 2^(logN+1)), no special primes
    OwnedContext(uint64_t T, int logN, int device) : OwnedContext(Parameters::FromModuli(logN, {T}, {}, T), device) {}
    OwnedContext(OwnedContext &&o) noexcept : ctx_(o.ctx_) { o.ctx_ = nullptr; }
    OwnedContext &operator=(OwnedContext &&o) noexcept;
    ~OwnedContext();
    OwnedContext Clone() const; // lumen_ctx_clone: the same tables and keys, its own streams and scratch
    lumen_ctx *get() const { return ctx_; }
    void check(int rc, const char *what) const; // throws std::runtime_error with lumen_last_error

  private:
    lumen_ctx *ctx_ = nullptr;
};
// test hook: the number of contexts the mirror's OwnedContexts hold at this moment
size_t LiveContextsForTest();

// []*rlwe.Ciphertext resident in HBM
class Ciphertexts {
  public:
    Ciphertexts() = default;
    Ciphertexts(lumen_ctx *ctx, lumen_set *set, MetaData md = MetaData()) : Meta(md), ctx_(ctx), set_(set) {}
    Ciphertexts(Ciphertexts &&o) noexcept { *this = std::move(o); }
    Ciphertexts &operator=(Ciphertexts &&o) noexcept;
    Ciphertexts(const Ciphertexts &) = delete;
    ~Ciphertexts();
    static Ciphertexts Upload(ServerBFV &backend, const std::vector<uint64_t> &host, int count, int level);
    std::vector<uint64_t> Download() const; // [count][2][level+1][N]
    int Len() const;
    int Level() const;
    lumen_set *Handle() const { return set_; }
    // gives the set up without destroying it (the caller re-wraps it, e.g. under another context of the same GPU)
    lumen_set *Release() {
        lumen_set *s = set_;
        set_ = nullptr, ctx_ = nullptr;
        return s;
    }
    lumen_ctx *Context() const { return ctx_; }
    MetaData Meta;
    uint64_t Scale() const { return Meta.Scale; }

  private:
    lumen_ctx *ctx_ = nullptr;
    lumen_set *set_ = nullptr;
};

// []*rlwe.Ciphertext spread over the ranks of a ServerGroup in contiguous blocks: block r (columns
// [r*Len/W, (r+1)*Len/W)) is resident on rank r's GPU.  One block = an ordinary slice on one GPU; the proof's
// MatR / MatZ are of this type either way, and the wire format is the blocks' ciphertexts in order.
struct ShardedCiphertexts {
    std::vector<Ciphertexts> Blocks;
    ShardedCiphertexts() = default;
    explicit ShardedCiphertexts(Ciphertexts one) { Blocks.push_back(std::move(one)); }
    int Len() const;
    int Level() const { return Blocks.empty() ? -1 : Blocks[0].Level(); }
    const MetaData &Meta() const;
    uint64_t Scale() const { return Meta().Scale; }
    std::vector<uint64_t> Download() const; // the blocks in order: [Len][2][level+1][N]
};

// Ciphertexts under the secret key in seeded form (lumen_encrypt_sk_seeded): c1 of ciphertext i is pure randomness,
// regenerated from the PUBLIC seed ASeed and the index FirstIndex + i, so only the c0 halves travel -- half the bytes of
// the witness upload.  ServerBFV::ExpandSeeded rebuilds the full top-level set with no key.  An in-memory object: there
// is no wire format for it yet.
struct SeededCiphertexts {
    std::array<uint8_t, 32> ASeed{};
    uint64_t FirstIndex = 0;
    int Count = 0;
    std::vector<uint64_t> C0; // [Count][L][N], NTT domain
};

// lintrans.LinearTransformation ([LATTIGO-RECALL] NewLinearTransformation + EncodeLinearTransformation, either form): the
// diagonals of a plaintext matrix, encoded over Q and P at one level and resident on the device as the multipliers of
// lumen_linear_transform (lumen_lintrans_load; lumen_lintrans_load_bsgs for the baby-step / giant-step form, pre-rotated
// there).  ServerBFV::NewLinearTransformation[BSGS] makes one; it owns the device object, is move-only and must not outlive
// the server it was made on (CopyNews of that server may apply it).
class LinearTransformation {
  public:
    LinearTransformation() = default;
    LinearTransformation(LinearTransformation &&o) noexcept { *this = std::move(o); }
    LinearTransformation &operator=(LinearTransformation &&o) noexcept;
    LinearTransformation(const LinearTransformation &) = delete;
    ~LinearTransformation();
    int Level() const { return level_; }
    // the keys the evaluation needs ([LATTIGO-RECALL] LinearTransformation.GaloisElements(params)): the Galois elements of the
    // non-zero diagonals, in ascending order of the diagonal's index; of a BSGS transformation, those of its baby steps
    // and then of its giant steps, each ascending
    std::vector<uint64_t> GaloisElements() const;
    const lumen_lintrans *Handle() const { return lt_; }

  private:
    friend class ServerBFV;
    lumen_ctx *ctx_ = nullptr;
    lumen_lintrans *lt_ = nullptr;
    int level_ = -1;
    size_t diagonals_ = 0;
};

// Scale after `for ct.Level() > target { Rescale }` from level `from`: scale * prod q_l^-1 mod T
uint64_t RescaledScale(const Parameters &params, uint64_t scale, int fromLevel, int toLevel);
// The MetaData block rlwe.Ciphertext.WriteTo puts in front of the polynomials, as recalled
// [LATTIGO-RECALL rlwe/metadata.go: MarshalBinary = MarshalJSON of {PlaintextMetaData, CiphertextMetaData},
// booleans and log-dimensions as "0x%02x" strings, Scale as {Value, Mod}]; a Go host replaces it with the
// real bytes (lumen_leaf_format_set).
std::string MetaDataJSON(const MetaData &md, uint64_t plaintextModulus);
// installs head = MetaData | LE64(2), poly_head = LE64(level+1), limb_head = LE64(N) on the backend
void SetCiphertextFormat(ServerBFV &backend, const MetaData &md, int level);

// The linear operations of the *bgv.Evaluator that both ServerBFV (fhe/bfv.go:13-21) and ClientBFV (bfv.go:60-81) embed,
// on whole slices (include/lumenos_hip.h, "the evaluator's linear operations"): the calls fhe/ntt.go:27-236 and
// vdec/batching.go:24-34 make.  One implementation over the owner's context; ServerBFV and ClientBFV inherit it.
// The ...New forms return a new slice.  The forms with `out` write an existing slice of the result's shape -- which may
// be one of the operands, as in backend.Add(batchCt, t, batchCt) -- or fill an empty one.  An operand of one ciphertext
// meets every ciphertext of the other; operands of different levels give the lower level (Lattigo's min-level rule).
// MetaData: the result takes the first operand's; Mul by a scalar keeps the scale; a plaintext product multiplies the
// scales modulo T.  RECORDED DEVIATION: Add and Sub require equal Scale() and throw std::invalid_argument
// naming both scales otherwise, where Lattigo would match the scales by a multiplication; MulThenAdd(ct, pt, acc)
// requires acc.Scale() == ct.Scale() * pt.Scale mod T.  MulCounter() is the library's: Mul / MulNew by a scalar or a
// plaintext count, Add, Sub and MulThenAdd do not (bfv.go:34-42 wraps Mul and MulNew alone).
class LinearEvaluator {
  public:
    virtual ~LinearEvaluator() = default;
    virtual lumen_ctx *Context() const = 0;
    virtual const Parameters &GetParameters() const = 0;
    virtual void check(int rc, const char *what) const = 0;
    Ciphertexts AddNew(const Ciphertexts &a, const Ciphertexts &b);
    void Add(const Ciphertexts &a, const Ciphertexts &b, Ciphertexts &out);
    Ciphertexts SubNew(const Ciphertexts &a, const Ciphertexts &b);
    void Sub(const Ciphertexts &a, const Ciphertexts &b, Ciphertexts &out);
    // Evaluator.Add / Sub(ct, pt): c0 +- pt; pt at ct's level or above (its first limbs are taken), of ct's scale
    Ciphertexts AddNew(const Ciphertexts &ct, const Plaintext &pt);
    void Add(const Ciphertexts &ct, const Plaintext &pt, Ciphertexts &out);
    Ciphertexts SubNew(const Ciphertexts &ct, const Plaintext &pt);
    void Sub(const Ciphertexts &ct, const Plaintext &pt, Ciphertexts &out);
    // Evaluator.Mul(ct, uint64): the scalar is w mod T, centred (the raw words of RootForwardUint64 go in as they are)
    Ciphertexts MulNew(const Ciphertexts &ct, uint64_t w);
    void Mul(const Ciphertexts &ct, uint64_t w, Ciphertexts &out);
    // Evaluator.MulNew(ct, pt) (lumen_mul_plain): pt at ct's level or above
    Ciphertexts MulNew(const Ciphertexts &ct, const Plaintext &pt);
    // Evaluator.MulThenAdd(ct, uint64 | pt, acc): acc += ct * operand, in place; acc may not be ct
    void MulThenAdd(const Ciphertexts &ct, uint64_t w, Ciphertexts &acc);
    void MulThenAdd(const Ciphertexts &ct, const Plaintext &pt, Ciphertexts &acc);
    // sum_t w[t] * in[t] for 1 to 8 slices of one scale, in one pass over the device (lumen_linear_combination)
    Ciphertexts LinearCombinationNew(const std::vector<const Ciphertexts *> &in, const std::vector<uint64_t> &w);

  private:
    void finish(lumen_set *set, const MetaData &md, Ciphertexts &out);
    const uint64_t *limbs_for(const char *what, const Ciphertexts &ct, const Plaintext &pt) const;
    void plain_sum(const char *what, const Ciphertexts &ct, const Plaintext &pt, Ciphertexts &out, bool sub);
};

// fhe.ServerBFV (fhe/bfv.go:13-58): plaintext field + parameters + evaluator/encoder/encryptor
class ServerBFV : public LinearEvaluator {
  public:
    // NewBackendBFV(plaintextField, params, pk, evk).  pk: [2][L][N] NTT domain; evk: Galois keys in
    // the layout of lumen_load_galois_key.
    ServerBFV(core::PrimeField *plaintextField, const Parameters &params, std::vector<uint64_t> pk,
              const std::map<uint64_t, std::vector<uint64_t>> &evk, int device = 0);
    // the same from a posted key set (cmd/server/main.go:100-140 after unmarshalling): keys.GaloisElements must be
    // params.GaloisElementsForInnerSum(1, rows); the keys go to the device in keys.Flags' form (lumen_load_galois_key_ex),
    // the relinearisation key too when the set carries one (SetRelinearizationKey)
    static std::unique_ptr<ServerBFV> NewFromKeySet(core::PrimeField *plaintextField, const Parameters &params, int rows,
                                                    const KeySet &keys, int device = 0);
    // the same from a seeded set (the `/keys` handler of cmd/server/main.go:66 at half the body): keys.GaloisB must hold
    // every element of params.GaloisElementsForInnerSum(1, rows); the relinearisation key too when the set carries one
    static std::unique_ptr<ServerBFV> NewFromKeySet(core::PrimeField *plaintextField, const Parameters &params, int rows,
                                                    const SeededKeySet &keys, int device = 0);
    // the switching keys of a seeded set, beside or over whatever is loaded: each key's `a` half is drawn on the device
    // under keys.ASeed.  A seeded key and a full key of one element replace each other.  keys.Pk is not looked at.
    void LoadSeededKeys(const SeededKeySet &keys);
    ~ServerBFV();
    core::PrimeField *Field() { return ptField_; }
    const Parameters &GetParameters() const { return params_; }
    int MulCounter() const; // bfv.go:44-46
    lumen_ctx *Context() const { return ctx_.get(); }
    // the rlwe.RelinearizationKey of the evaluation key set (bfv.go:23-28: NewMemEvaluationKeySet(rlk, galoisKeys...)),
    // [beta][b|a][L+K][N] as KeyGenerator::GenRelinearizationKeyNew(flags) returns it; CopyNews share it; setting it again
    // replaces it (lumen_load_relin_key)
    void SetRelinearizationKey(const std::vector<uint64_t> &rlk, uint32_t flags = 0);
    // Evaluator.MulRelinNew over an rlwe.Operand that is a ciphertext (bfv.go:34-42): a[i] * b[i], or a[i] * b[0] when b
    // holds one ciphertext; a and b of one level (a and b may be the same object: squares).  The result's Scale() is
    // a.Scale() * b.Scale() mod T; MulCounter() grows by a.Len().  Needs the relinearisation key.
    Ciphertexts MulRelinNew(const Ciphertexts &a, const Ciphertexts &b);
    // Sums of n products with ONE relinearisation each -- Evaluator.MulNew(a_0, b_0), MulThenAdd(a_i, b_i, acc) for the
    // other terms, Relinearize(acc) --: out[g] = sum_i a[g n + i] * b[g n + i] when b has a's count, sum_i a[g n + i] * b[i]
    // when b holds n ciphertexts (matrix x vector).  One level, a and b may be the same object; Scale() and the key are
    // MulRelinNew's, MulCounter() grows by a.Len().  std::invalid_argument: empty operands, n == 0, a.Len() no multiple of
    // n, b.Len() neither a.Len() nor n, different levels (lumen_mul_relin_dot).
    Ciphertexts DotRelinNew(const Ciphertexts &a, const Ciphertexts &b, uint32_t n);
    // Galois keys for arbitrary elements, beside whatever the constructor loaded (evk.GaloisKeys of an
    // rlwe.MemEvaluationKeySet holds any element the client generated): element -> [beta][b|a][L+K][N] as
    // KeyGenerator::GenGaloisKeysNew returns them, in `flags`' form.  CopyNews share them; loading an element again replaces its key.
    void LoadGaloisKeys(const std::map<uint64_t, std::vector<uint64_t>> &keys, uint32_t flags = 0);
    // The rotations of the embedded *bgv.Evaluator (bfv.go:13-21), on every ciphertext of `ct` at its level; the result
    // keeps ct's MetaData (a rotation leaves the scale alone) and MulCounter() does not move.  Each needs the Galois key of
    // its element (the identity needs none and copies).
    // Evaluator.Automorphism(ct, galEl, opOut) into a new set
    Ciphertexts AutomorphismNew(const Ciphertexts &ct, uint64_t galEl);
    // Evaluator.RotateColumnsNew(ct, k): slot i of both rows takes the value of slot i + k (mod N/2)
    Ciphertexts RotateColumnsNew(const Ciphertexts &ct, int k);
    // Evaluator.RotateRowsNew(ct): the two rows of N/2 slots change places
    Ciphertexts RotateRowsNew(const Ciphertexts &ct);
    // Evaluator.RotateHoistedNew(ct, rotations): rotation -> RotateColumnsNew(ct, rotation), the decomposition of c1 done
    // once (lumen_rotate_hoisted); at most 64 distinct rotations
    std::map<int, Ciphertexts> RotateHoistedNew(const Ciphertexts &ct, const std::vector<int> &rotations);
    // Evaluator.InnerSum(ct, batchSize, n, opOut) into a new set (lumen_inner_sum_general): slot j of each row takes
    // sum_{i < n} slot[j + i * batchSize]; any n with batchSize * n <= N / 2, and batchSize 1 with n a power of two <= N.
    // Needs the Galois keys of a subset of GaloisElementsForInnerSum(batchSize, n).
    Ciphertexts InnerSumNew(const Ciphertexts &ct, int batchSize, int n);
    // The diagonal method on the embedded evaluator (bfv.go:13-21; [LATTIGO-RECALL] lintrans Evaluator.LinearTransformationNew /
    // LinearTransformationsNew, the non-BSGS branch): out = sum_k diag_k (.) RotateColumns(ct, k), single-hoisted with ONE
    // ModDown for the sum (lumen_linear_transform).  diagonals: k -> up to N slot values, |k| < N/2; level: the level of the
    // ciphertexts it will meet.  ct at the transform's level; the result keeps ct's MetaData (Encode leaves scale 1) and
    // MulCounter() does not move.  Needs the Galois keys of lt.GaloisElements() (KeyGenerator::GenGaloisKeysNew,
    // LoadGaloisKeys); diagonal 0 alone needs none.  Column rotations only, at most two special primes.
    // NewLinearTransformationBSGS: the double-hoisted form (the BSGS branch, MultiplyByDiagMatrixBSGS) of the same diagonals
    // with babySteps baby steps, 0 for the count with the fewest keys (lumen_lintrans_best_baby_steps): about
    // babySteps + D / babySteps keys and gadget products for D diagonals.  The evaluation calls are the same.
    LinearTransformation NewLinearTransformation(const std::map<int, std::vector<uint64_t>> &diagonals, int level);
    LinearTransformation NewLinearTransformationBSGS(const std::map<int, std::vector<uint64_t>> &diagonals, int level, int babySteps);
    Ciphertexts LinearTransformationNew(const Ciphertexts &ct, const LinearTransformation &lt);
    std::vector<Ciphertexts> LinearTransformationsNew(const Ciphertexts &ct, const std::vector<const LinearTransformation *> &lts);
    // Encoder.Encode(values, pt) at MaxLevel ([LATTIGO-RECALL] m * T^-1 form, slot index matrix)
    Plaintext Encode(const std::vector<uint64_t> &values) const;
    // the same extended to the limbs modulo P, at `level`: Value is [level + 1 limbs of Q][K limbs of P][N], every
    // coefficient's lift in [0, T) and the factor T^-1 as in Encode -- a diagonal as lumen_lintrans_load takes it
    Plaintext EncodeQP(const std::vector<uint64_t> &values, int level) const;
    // Encryptor.EncryptNew(pt) under pk, host layout [2][L][N]
    std::vector<uint64_t> EncryptNew(const Plaintext &pt);
    // the same for a batch of MaxLevel plaintexts, on the device (lumen_encrypt_pk): the witness
    // encryption loop of cmd/server/main.go:199-208; the result stays in HBM
    Ciphertexts EncryptNewBatch(const std::vector<Plaintext> &pts);
    // Encoder.Encode + EncryptNew of `count` columns of `rows` values ([count][rows]), both on the device
    Ciphertexts EncryptColumnsNew(const std::vector<uint64_t> &values, int rows, int count);
    // the claimed value of GET /prove?point=z (cmd/server/main.go:255-258: core.NewDensePolyFromMatrix(matrix).Evaluate)
    // over `count` witness columns of `rows` values ([count][rows], what EncryptColumnsNew takes) that begin at column
    // `firstColumn` of a matrix of `cols` columns, on the device (lumen_poly_eval_columns): the whole matrix gives
    // P(z), disjoint column blocks give partials that sum mod T to it.  Prints the reference's span
    // "Evaluate polynomial".
    core::Element EvaluateColumns(const std::vector<uint64_t> &values, int rows, int count, int cols, core::Element z,
                                  uint64_t firstColumn = 0);
    // the server's side of a client's seeded upload (lumen_ct_expand_seeded): c0 halves + public seed -> the full
    // top-level ciphertexts, ready for LigeroCommitter::Commit.  Needs no key.
    Ciphertexts ExpandSeeded(const SeededCiphertexts &seeded);
    void check(int rc, const char *what) const; // throws std::runtime_error with lumen_last_error
    void SetRingSwitchServer(RingSwitchServer *rs) { rs_ = rs; } // bfv.go:48-50
    RingSwitchServer *RingSwitch() const { return rs_; }          // bfv.go:52-54
    // ServerBFV.CopyNew (bfv.go:56-58): Evaluator.ShallowCopy -- the same parameters, keys and ENCRYPTOR (the Go
    // copy shares the pointer: seed and position in its stream), its own scratch: a lumen_ctx_clone on the same
    // GPU.  What a goroutine that evaluates concurrently takes (ligero.go:142, 315), and what plays a rank of a
    // ServerGroup when several ranks share one GPU.  The copy must not outlive the server it was made from.
    std::unique_ptr<ServerBFV> CopyNew();

  private:
    ServerBFV(ServerBFV &src, OwnedContext clone);
    Plaintext encode_limbs(const std::vector<uint64_t> &values, int level, bool withP) const;
    LinearTransformation newLinearTransformation(const std::map<int, std::vector<uint64_t>> &diagonals, int level, int babySteps,
                                                 const char *what);
    friend class ServerGroup;
    core::PrimeField *ptField_;
    Parameters params_;
    std::vector<uint64_t> pk_;
    OwnedContext ctx_;
    uint64_t psiT_ = 0;
    std::vector<uint32_t> slot_index_;
    RingSwitchServer *rs_ = nullptr;
    // the encryptor's state, shared with every CopyNew and by the ranks of a ServerGroup: the ChaCha20 key of
    // every sample drawn (OsRandom, never a PRNG) and the index of the next ciphertext in its stream
    struct EncryptorState {
        uint8_t seed[32] = {0};
        std::atomic<uint64_t> next{0};
    };
    std::shared_ptr<EncryptorState> enc_;

  public:
    // test hooks: the seed must differ between instances (it is the only secret of the encryptor); rewinding the
    // stream lets a test encrypt the same witness twice to the same bits (one GPU against a group)
    const uint8_t *EncSeedForTest() const { return enc_->seed; }
    void RewindEncryptorForTest(uint64_t next = 0) { enc_->next = next; }
};

// fhe.ClientBFV (fhe/bfv.go:60-106): plaintext field + parameters + encoder / decryptor under the secret key, for a
// client that owns a GPU: a context with lumen_encoder_set and a secret key.  The key is either handed in (sk: [L][N] or
// [L+K][N], NTT domain, what lumen_load_secret_key takes) or GENERATED ON THE DEVICE (NewWithGeneratedSecret:
// lumen_keygen_secret under a 32-byte seed from getrandom(2)); a client of the second kind is what fhe::KeyGenerator
// and NewRingSwitchClient derive the public, relinearisation, Galois and ring-switch keys from.
class ClientBFV : public LinearEvaluator { // (the reference's ClientBFV embeds an evaluator too: vdec.BatchCiphertexts runs on it)
  public:
    // NewClientBFV(plaintextField, paramsFHE, sk)
    ClientBFV(core::PrimeField *plaintextField, const Parameters &params, const std::vector<uint64_t> &sk, int device = 0);
    // kgen.GenSecretKeyNew() + NewClientBFV (cmd/client/main.go:74-76, 90): the secret never leaves the device.  The
    // seed is key material: it comes from the kernel's CSPRNG, as ServerBFV's encryptor seed does, and keys nothing else.
    static std::unique_ptr<ClientBFV> NewWithGeneratedSecret(core::PrimeField *plaintextField, const Parameters &params,
                                                             int device = 0);
    ~ClientBFV();
    ClientBFV(const ClientBFV &) = delete;
    core::PrimeField *Field() { return ptField_; }
    const Parameters &GetParameters() const { return params_; }
    lumen_ctx *Context() const { return ctx_.get(); }
    int Device() const { return device_; }
    int MulCounter() const; // the library's counter of this client's context
    void check(int rc, const char *what) const; // throws std::runtime_error with lumen_last_error
    // ClientBFV.CopyNew (bfv.go:96-98): the same key and tables, its own streams and scratch (lumen_ctx_clone); must
    // not outlive the client it was made from
    std::unique_ptr<ClientBFV> CopyNew();
    // the rlwe.NewEncryptor(paramsFHE, sk) of fhe/bfv.go:77, on the device (lumen_encrypt_sk_*): Encoder.Encode +
    // EncryptNew of `count` columns of `rows` values ([count][rows]) under the client's secret key.  The error seed is
    // key material drawn once per client from getrandom(2) (CopyNews share it); every call draws a FRESH public seed for
    // c1 from getrandom(2), so no (seed, index) pair ever encrypts two messages.
    Ciphertexts EncryptColumnsNew(const std::vector<uint64_t> &values, int rows, int count);
    // the same ciphertexts in seeded form: what the client uploads (c0 halves + the public seed)
    SeededCiphertexts EncryptColumnsSeeded(const std::vector<uint64_t> &values, int rows, int count);
    // test hook: the full ciphertexts under a GIVEN public seed and first index -- to compare a server's ExpandSeeded
    // against, never to encrypt anything else
    Ciphertexts EncryptColumnsUnderSeedForTest(const std::vector<uint64_t> &values, int rows, int count,
                                               const std::array<uint8_t, 32> &aSeed, uint64_t firstIndex);
    bool HasGeneratedSecret() const { return (bool)keySeed_; }
    // the seed of a generated secret (what the KeyGenerator passes on); throws for a client that was handed its key
    const uint8_t *KeySeed() const;
    // The PUBLIC seed of this client's seeded switching keys: drawn once, together with the keygen seed, shared with every
    // CopyNew and used for every SeededKeySet.  Throws for a client that was handed its key.
    const std::array<uint8_t, 32> &PublicKeySeed() const;
    // One `a` per key, enforced: records that the keys `keyIds` (the sampling contract's ids: 2 = relinearisation,
    // 0x10000 + g = Galois element g) leave this client in the seeded (or the full) form and throws std::logic_error,
    // before anything is generated, if one of them already left it in the other form -- the full form's a is drawn under
    // the keygen seed, the seeded form's under PublicKeySeed(), and both keys together reveal the secret.  The same form
    // again is the same words and is allowed.  KeyGenerator calls it; shared with every CopyNew.
    void ClaimKeyForm(const std::vector<uint64_t> &keyIds, bool seeded);
    // test hook: the generated secret as [L+K][N] NTT-domain residues (regenerated from the seed into a host buffer:
    // the one way it leaves the device)
    std::vector<uint64_t> SecretKeyForTest();

  private:
    ClientBFV(core::PrimeField *plaintextField, const Parameters &params, int device);
    ClientBFV(ClientBFV &src, OwnedContext clone);
    core::PrimeField *ptField_;
    Parameters params_;
    OwnedContext ctx_;
    int device_ = 0;
    struct KeySeedBytes {
        uint8_t b[32];
    };
    std::shared_ptr<KeySeedBytes> keySeed_; // shared with every CopyNew
    struct KeyForms { // what belongs to keySeed_ beyond its bytes; shared with every CopyNew
        std::array<uint8_t, 32> aSeed{};
        std::mutex mu;
        std::map<uint64_t, bool> seeded; // key id -> the form it was generated in
    };
    std::shared_ptr<KeyForms> keyForms_;
    std::shared_ptr<KeySeedBytes> encSeed_; // the encryptor's error seed, shared with every CopyNew; keys nothing else
};

// rlwe.NewKeyGenerator(params) (cmd/client/main.go:74) bound to a client with a generated secret: every key is derived
// on the device from the client's seed (include/lumenos_hip.h, "SAMPLING CONTRACT"), so generating a key twice, one
// at a time or in a batch gives the same words.  flags: 0 or LUMEN_KEY_MONTGOMERY.
// A switching key leaves a client in ONE form, full or seeded (ClientBFV::ClaimKeyForm): asking for the other form of a key
// already generated throws std::logic_error.
class KeyGenerator {
  public:
    explicit KeyGenerator(ClientBFV &client); // throws std::invalid_argument for a client that was handed its key
    // GenKeyPairNew(): the secret is the client's own and stays where it is; returns pk, [2][L+K][N]
    std::vector<uint64_t> GenKeyPairNew();
    // GenRelinearizationKeyNew(sk): [beta][b|a][L+K][N]
    std::vector<uint64_t> GenRelinearizationKeyNew(uint32_t flags = 0);
    // GenGaloisKeysNew(galEls, sk): one launch of each kernel and one transfer for all the (distinct) elements
    std::map<uint64_t, std::vector<uint64_t>> GenGaloisKeysNew(const std::vector<uint64_t> &galEls, uint32_t flags = 0);
    // pk + the Galois keys of params.GaloisElementsForInnerSum(1, rows) in that order: the body of POST /keys
    // withRelin: the set carries the relinearisation key as well, as the reference's /keys body does
    KeySet GenKeySetNew(int rows, uint32_t flags = 0, bool withRelin = false);
    // GenGaloisKeysNew in seeded form: a set under the client's PublicKeySeed() (never its secret seed, never a second one) holding
    // the b halves of the (distinct) elements, one launch of each kernel and one transfer of half the size
    SeededKeySet GenGaloisKeysSeeded(const std::vector<uint64_t> &galEls, uint32_t flags = 0);
    // GenRelinearizationKeyNew in seeded form, INTO a set of this client's: its b half under the set's Flags.  An empty
    // (default-constructed) set takes the client's PublicKeySeed(); a set under another seed is refused (std::invalid_argument).
    void GenRelinearizationKeySeeded(SeededKeySet &set);
    // pk + the seeded Galois keys of params.GaloisElementsForInnerSum(1, rows): what NewFromKeySet(., SeededKeySet) takes
    SeededKeySet GenKeySetSeeded(int rows, uint32_t flags = 0, bool withRelin = false);

  private:
    ClientBFV &client_;
};

// fhe.NewRingSwitchClient (fhe/ring_switch.go:16-57): the small-ring secret skNew (2^logN ternary coefficients) and the
// evaluation key sk -> skNew(X^(N/n)), [rns][pw2][b|a][L+K][N] as NewRingSwitchServer / lumen_load_ringswitch_key take it
struct RingSwitchClient {
    int LogN = 0, BaseTwoDecomposition = 13;
    std::vector<int8_t> SkNew;
    std::vector<uint64_t> Evk;
};
RingSwitchClient NewRingSwitchClient(ClientBFV &client, int logN, int baseTwoDecomposition = 13);

// W = 2^k ServerBFVs behind one lumen_group (include/lumenos_hip.h): the ranks of ONE server process that owns
// several GPUs -- the reference's server is a single process (cmd/server/main.go:187-266).  ranks[r] is rank r;
// they hold the same parameters, public key and evaluation keys (one NewBackendBFV per GPU, or CopyNew()s of one
// server when ranks share a GPU).  The group makes them ONE encryptor: every rank draws from rank 0's stream, so
// a column encrypts to the same bits on whichever GPU it lands.
class ServerGroup {
  public:
    explicit ServerGroup(std::vector<ServerBFV *> ranks, uint32_t transport = LUMEN_TRANSPORT_AUTO);
    ~ServerGroup();
    ServerGroup(const ServerGroup &) = delete;
    int World() const { return (int)ranks_.size(); }
    ServerBFV &Rank(int r) const { return *ranks_.at((size_t)r); }
    lumen_group *Handle() const { return group_; }
    std::string Transport() const { return lumen_group_transport(group_); }
    std::string TransportNote() const { return lumen_group_transport_note(group_); } // how it was chosen (librccl version, fall-back reason ...)
    void check(int rc, const char *what) const; // throws std::runtime_error with lumen_last_error(NULL)
    void Sync() const;
    // the witness encryption loop of cmd/server/main.go:188-208 over the ranks: column j (of `count`, `rows`
    // values each) is encoded and encrypted on rank j / (count/W), with its own place in the encryptor's stream
    ShardedCiphertexts EncryptColumnsNew(const std::vector<uint64_t> &values, int rows, int count);
    // P(z) of the same witness over the ranks (lumen_group_poly_eval): rank r evaluates the block of columns
    // EncryptColumnsNew puts on it, the partials are summed inside the library.  Prints "Evaluate polynomial".
    core::Element EvaluateColumns(const std::vector<uint64_t> &values, int rows, int count, int cols, core::Element z);

  private:
    std::vector<ServerBFV *> ranks_;
    lumen_group *group_ = nullptr;
};

// n bytes from the kernel CSPRNG (getrandom(2)); throws if unavailable
void OsRandom(uint8_t *out, size_t n);

// fhe.RingSwitchServer (fhe/ring_switch.go:93-113)
class RingSwitchServer {
  public:
    // NewRingSwitchServer(ringSwitchEvk, paramsLit): paramsLit.LogN is the target degree, its single
    // modulus is q_0 (ring_switch.go:30-38); ringSwitchEvk is the whole evaluation key the client posts,
    // flattened [rns][pw2][b|a][L+K][N] (lumen_load_ringswitch_key; RNS digit 0 alone is accepted too)
    RingSwitchServer(ServerBFV &backend, const std::vector<uint64_t> &ringSwitchEvk, int logN,
                     int baseTwoDecomposition = 13);
    // RingSwitchNew for every ciphertext of the slice: host result [len][2][2^logN] (level 0, small ring)
    std::vector<uint64_t> RingSwitchNew(const Ciphertexts &cts, ServerBFV &backend) const;
    int LogN() const { return logN_; }

  private:
    int logN_;
};

// fhe.Encode (fhe/code.go:8-34)
Ciphertexts Encode(const Ciphertexts &matrix, int rows, int rhoInv, ServerBFV &backend);
// the same over a group: matrix.Blocks[r] = rank r's columns; the lane-sharded transform between two all-to-alls
// (lumen_group_encode), byte-identical to Encode on one GPU
ShardedCiphertexts Encode(const ShardedCiphertexts &matrix, int rows, int rhoInv, ServerGroup &group);
// fhe.NTT (fhe/ntt.go:12-18): in place on `values`
void NTT(Ciphertexts &values, int size, ServerBFV &backend);

struct LigeroMetadata { // fhe/ligero.go:19-24
    int Rows = 0, Cols = 0, RhoInv = 0, Queries = 0;
    void WriteTo(std::vector<uint8_t> &buf) const; // ligero.go:755-761
};

int calculateQueries(double securityBits, int rhoInv); // ligero.go:65-71

// page-locked host bytes (lumen_host_alloc): where a proof's wire image is assembled -- the device writes it
// by DMA, and a Go []byte over the same memory feeds the HTTP response (cmd/server/main.go:154-171)
class WireBuffer {
  public:
    WireBuffer() = default;
    explicit WireBuffer(size_t n);
    WireBuffer(WireBuffer &&o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr, o.n_ = 0; }
    WireBuffer &operator=(WireBuffer &&o) noexcept;
    WireBuffer(const WireBuffer &) = delete;
    ~WireBuffer();
    uint8_t *data() const { return p_; }
    size_t size() const { return n_; }

  private:
    uint8_t *p_ = nullptr;
    size_t n_ = 0;
};

// go-humanize Bytes(): what the reference prints for its marshaled sizes (ligero.go:672,682,692)
std::string HumanizeBytes(uint64_t s);

struct EncryptedProof { // fhe/ligero.go:185-192
    LigeroMetadata Metadata;
    ShardedCiphertexts MatR, MatZ; // one block on one GPU; with a ServerGroup block r is resident on rank r
    Ciphertexts QueriedCols;
    // with a ring switch (ligero.go:336-342) MatR / MatZ are level-0 ciphertexts of the small ring instead:
    // host residues [cols][2][2^RingSwitchLogN] (what RingSwitchNew returns), MetaData as the inputs'
    std::vector<uint64_t> MatRSwitched, MatZSwitched;
    int RingSwitchLogN = 0;
    std::vector<std::vector<core::Digest>> MerklePaths;
    std::vector<uint8_t> Root;
    std::vector<int> QueryIndices; // not part of the wire format; kept for tests
    uint64_t PlaintextModulus = 0;
    // ligero.go:646-705 (MarshalBinary = WriteTo into a buffer): metadata | MatR | MatZ | QueriedCols | paths |
    // root, every ciphertext as ct.WriteTo emits it in the recalled framing (MetaDataJSON | LE64(2) | per
    // polynomial LE64(limbs) | per limb LE64(N) | words).  The images of the three slices are assembled on the
    // device (lumen_ct_serialize_async) and arrive by DMA.  Prints the reference's three "Marshaled ...: size" lines.
    size_t MarshaledSize() const;
    void MarshalInto(uint8_t *out, size_t cap, bool pageLocked) const;
    std::vector<uint8_t> MarshalBinary() const; // pageable memory: bounce-buffered, slower
    WireBuffer MarshalBinaryPinned() const;     // page-locked memory: the fast path
    // EncryptedProof.UnmarshalBinary / ReadFrom (ligero.go:654-753): the three slices' images go to the device
    // as they are (lumen_ct_deserialize takes them apart there and checks the framing); level-1 ciphertexts of
    // the backend's parameters (a ring-switched proof is read by the client's small-ring parameters, not here).
    // `meta`: the MetaData the ciphertexts carry (what SetCiphertextFormat frames them with).
    static EncryptedProof UnmarshalBinary(const uint8_t *data, size_t len, ServerBFV &backend, const MetaData &meta);
    // the same on the client's context (cmd/client/main.go:181-184): what Decrypt then reads
    static EncryptedProof UnmarshalBinary(const uint8_t *data, size_t len, ClientBFV &client, const MetaData &meta);
    // EncryptedProof.Decrypt (ligero.go:381-502) on the client's device, under the reference's spans "Decrypt queried
    // columns" (lumen_decrypt of every opened column, `rows` values each) and "Decrypt row inner products" (MatR and
    // MatZ, one value per ciphertext: decodeSingleElement).  The opened ciphertexts stay on the device and move into
    // the proof (ColumnInstance.Ct), so this EncryptedProof gives them up.  A ring-switched proof is refused with a
    // message (the reference's client skips Verify for it, cmd/client/main.go:210-212).
    Proof Decrypt(ClientBFV &client, core::Span *ctx);
};

class LigeroCommitter;

struct LigeroProver { // fhe/ligero.go:32-37
    const LigeroCommitter *Committer = nullptr;
    const Ciphertexts *Matrix = nullptr;
    const ShardedCiphertexts *MatrixShards = nullptr; // the same when Commit ran on a ServerGroup
    // DEVIATION from the reference's field (ligero.go:32-37, 117-123): there `EncodedMatrix` is the top-level
    // encoded matrix, whose queried entries Prove rescales IN PLACE to level 1 and aliases into the proof
    // (ligero.go:268-273).  Here Commit keeps the LEVEL-1 columns it hashed -- the only form Prove ever reads
    // (25.8 GB of top-level ciphertexts at 16384 x 4096 against 4.3 GB) -- hence the other name: a caller reading
    // it sees level-1 columns everywhere, not just at the queried indices.  Proof bytes are the same, and so is a
    // second Prove on the same prover (the reference's `for Level() > 1` finds nothing left to do on the columns
    // the first one touched): tests/cpp/test_ligero_host.cpp proves twice.
    ShardedCiphertexts EncodedLevel1;
    core::MerkleTree Tree;
    // ligero.go:231-242 evaluates the R and Z inner products CONCURRENTLY, each goroutine on its own
    // backend.CopyNew(); set this to do the same (two host threads, the server and a CopyNew of it: two streams on
    // the one GPU) -- the spans then overlap as the reference's do.  Default: one after the other on the server's
    // own context, which is what the span times of DESIGN.md section 6 are and, on one GPU, 4 % faster (two transform
    // kernels side by side evict each other's L2 sets).  The proof's bytes are the same either way.
    bool ConcurrentRZ = false;
    // ligero.go:194-291
    EncryptedProof Prove(core::Element point, ServerBFV &backend, core::Transcript &transcript, core::Span *ctx);
    // the same over the ranks of a group: inner products on every rank's own columns, the queried columns
    // collected on rank 0 (lumen_group_gather); the proof's bytes are those of the one-GPU run
    EncryptedProof Prove(core::Element point, ServerGroup &group, core::Transcript &transcript, core::Span *ctx);
};

class LigeroCommitter { // fhe/ligero.go:27-29, 40-63
  public:
    LigeroMetadata Metadata;
    static LigeroCommitter NewLigeroCommitter(double securityBits, int rows, int cols, int rhoInv);
    // ligero.go:95-124: returns the prover state and the Merkle root
    std::pair<LigeroProver, std::vector<uint8_t>> Commit(const Ciphertexts &matrix, ServerBFV &backend,
                                                         core::Span *ctx) const;
    // the same over the ranks of a group: Encode between two all-to-alls, every rank rescales and
    // hashes its block of encoded columns, ONE all-gather assembles the S leaf digests, the host keeps the tree
    std::pair<LigeroProver, std::vector<uint8_t>> Commit(const ShardedCiphertexts &matrix, ServerGroup &group,
                                                         core::Span *ctx) const;
};

// fhe.Proof (ligero.go:372-379): the plain prover's output (LigeroProveReference) and what EncryptedProof::Decrypt
// returns
struct Proof {
    LigeroMetadata Metadata;
    std::vector<uint8_t> Root;
    std::vector<uint64_t> MatR, MatZ;                  // one field element per column
    std::vector<std::vector<uint64_t>> QueriedCols;     // `rows` values of every opened encoded column (ColumnInstance.Values)
    std::vector<std::vector<core::Digest>> MerklePaths;
    std::vector<int> QueryIndices;                      // LigeroProveReference only (not part of a proof)
    // ColumnInstance.Ct of every opened column, in query order, resident on the client's device (Decrypt); empty for
    // LigeroProveReference, whose leaves are plain columns
    std::shared_ptr<Ciphertexts> QueriedCts;
    // Proof.Verify (ligero.go:517-574): the reference's order and its error strings, thrown as std::runtime_error --
    // sample r; core.Encode of MatR and MatZ; append the point; zPow; sample the query indices; the per-column loop
    // (Merkle path, <Values, r>, <Values, b>) as ONE lumen_verify_columns over QueriedCts; InnerProduct(MatZ, a) == value.
    // DEVIATION from the reference's signature: `client` is an extra argument.  There the loop reads the Values
    // Decrypt left on the host and hashes Ct's bytes on the host; here the opened columns are hashed AND decrypted
    // again inside the device check (their values never leave it), which needs the context that holds the secret key.
    // QueriedCols (the host copy Decrypt made for ProveDecrypt) is not read.  Paths of another length than the tree's
    // depth, or fewer paths than queries, are the Merkle failure of the first such query.
    void Verify(core::Element point, core::Element value, core::PrimeField &field, core::Transcript &transcript,
                ClientBFV &client) const;
    // Proof.ProveDecrypt (ligero.go:504-515) -> vdec.ProveBfvDecBatched (vdec/prover.go:50-98) up to the call into lazer,
    // under the reference's spans "Verifiable decrypt", "Batching decrypted columns", "Batching ciphertexts" and
    // "Witness generation", with the transcript "vdec": folds QueriedCols with the transcript's challenges on the host,
    // batches QueriedCts on the client's device (lumen_batch_ciphertexts), rescales to level 0 and returns the witness
    // (lumen_vdec_witness).  Stops where CallVdecProver would call ProveVdecLnpTbox: lazer is not part of this project.
    // THE BUDGET: a full-size plaintext costs about N * T in noise, so the batch only decrypts where
    // T * count * N * T * (B + 1) < Q_level / 2 (include/lumenos_hip.h; tools/noise_budget.py --vdec): the reference's
    // vdec tests use T = 0x3ee0001 for that reason.  The decryption relation is checked on the device: throws
    // std::runtime_error naming the budget when |err| * 2T >= q_0, and when QueriedCts is empty.
    vdec::Witness ProveDecrypt(ClientBFV &client, core::Span *ctx) const;
};
// the error Proof.Verify's loop returns for one column's status word of lumen_verify_columns (ligero.go:556, 561, 565:
// PATH before R before B); empty when the column passed
std::string VerifyColumnError(uint32_t status, int queryColIdx);
// core.Encode (core/code.go:3-23) of up to 512 rows of equal length at once, on the device: the rows are the lanes of
// a plain context whose one modulus is T (the path LigeroProveReference drives, at the smallest ring degree the
// library instantiates), one lumen_encode for all.  field: N() = len * rhoInv.  -> rows of len * rhoInv elements.
std::vector<std::vector<core::Element>> EncodeRows(const std::vector<std::vector<core::Element>> &rows, int rhoInv,
                                                   core::PrimeField &field, int device = 0);
// LigeroCommitter.LigeroProveReference (ligero.go:799-953): the prover without encryption, on the device
// through the same C ABI -- a context whose one modulus is T holds the matrix column by column
// (lumen_plain_inner_products's header comment).  matrix: row-major [rows][cols].
Proof LigeroProveReference(const LigeroCommitter &c, const std::vector<uint64_t> &matrix, core::Element point,
                           core::PrimeField &field, core::Transcript &transcript, int device = 0);

// matrixInnerSumEval (ligero.go:299-370), without the ring switch, at the level of `matrix` (the plaintext at the same
// level: the first Level + 1 limbs of an Encode)
Ciphertexts matrixInnerSumEval(const Ciphertexts &matrix, const Plaintext &plaintext, int rows, ServerBFV &backend);
std::vector<int> sampleQueryIndices(core::Transcript &transcript, int queries, int extCols); // ligero.go:638-644

} // namespace fhe

// the front end of the reference's `vdec` package (vdec/batching.go) above the C ABI
namespace vdec {
// vdec.BatchColumns (batching.go:43-64), on the host: one SampleUints("pod_alpha", rows words) per column, in column
// order; batchCol[i] = sum_j matrixColMajor[j][i] * alphas[j][i] mod T (a challenge word >= T counts as its residue).
// Returns (batchCol, alphasColMajor).
std::pair<std::vector<core::Element>, std::vector<std::vector<uint64_t>>>
BatchColumns(const std::vector<std::vector<core::Element>> &matrixColMajor, core::PrimeField &field, core::Transcript &transcript);
// vdec.BatchCiphertexts (batching.go:9-41) on the client's device (lumen_batch_ciphertexts): sum_j cts[j] * pt(alphas[j]),
// the plaintexts at the ciphertexts' scale (alphaPts[i].MetaData = cts[0].MetaData).  ONE ciphertext at the level of
// `cts`; its Scale is the square of theirs modulo T.
fhe::Ciphertexts BatchCiphertexts(const fhe::Ciphertexts &cts, const std::vector<std::vector<uint64_t>> &alphasColMajor,
                                  fhe::ClientBFV &client);
} // namespace vdec
} // namespace lumenos
